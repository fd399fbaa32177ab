"""Element-wise conformance of gvf_gemm's four-wave kernel (csrc/gemm.hip) and of the router in front of it, against the float64 reference
of tests/gemm_ref.py.  Every case checks (a) every output element within gemm_ref's bound, (b) nothing outside [M, N] of the output
written (a view inside a larger buffer pre-filled with NaN / a 16-bit sentinel, ldc > N, rows after M), (c) no read past K (A and W are
views whose padding columns hold NaN), (d) the same bits on a second launch.  The case matrix is pairwise over M (partial 64- and
128-row tiles), N (scalar stores, tails, multiples of 192), K (one k-tile, long K on 32-deep k-tiles, 64-deep k-tiles), the five
epilogues, gated and ungated residual updates with their row statistics, and the LayerNorm-folded operand.

The tile switches GVF_GEMM_BM / GVF_GEMM_BK / GVF_GEMM_BN192 / GVF_GEMM8 are read once per process: test_variants_forced_in_child_processes
re-runs this file with them set.  Row invariance: a row's bits do not depend on the other rows of the call inside the four-wave kernel
(whatever tile shape M selects), nor in DiT.prepare_conditions' condition products (whatever the batch)."""
import json
import math
import os
import subprocess
import sys

import pytest
import torch

import gemm_ref as G
from gvfdiffusion_amd import _lib, synthetic
from gvfdiffusion_amd.ops import dit_ops

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.environ.get("GVF_GEMM_CONFORMANCE_CHILD") == "1"
SENTINEL16 = 0x7E5A                  # a 16-bit pattern no kernel writes here (fp16: a NaN payload; bf16: 7.2e37)
DTYPES = [torch.bfloat16, torch.float16]
S16, GELU, F32, RESID, GEGLU = G.EPI_STORE_16, G.EPI_GELU_16, G.EPI_STORE_F32, G.EPI_RESID_F32, G.EPI_GEGLU_16


def _variant(M, N, K, epi):
    """The four-wave instantiation launch_gemm picks (csrc/gemm.hip), for the log."""
    tiles_n = (N + 127) // 128
    bm_env = int(os.environ.get("GVF_GEMM_BM", "0"))
    bm = (64 if bm_env == 64 else 128) if bm_env else (64 if ((M + 127) // 128) * tiles_n < 512 else 128)
    bk_env = int(os.environ.get("GVF_GEMM_BK", "0"))
    bk64 = bk_env == 64 if bk_env else K >= 1024
    bk = 64 if bk64 and K % 64 == 0 else 32
    mode = int(os.environ.get("GVF_GEMM_BN192", "1"))
    tiles_m = (M + bm - 1) // bm
    tail128, tail192 = (tiles_m * tiles_n) % 1024, (tiles_m * (N // 192)) % 768
    wide = bm == 128 and not bk64 and epi not in (GEGLU, RESID) and N % 192 == 0 and mode != 0 and \
        (mode == 2 or (0 < tail128 <= 256 and (tail192 == 0 or tail192 > 384)))
    return f"BM{bm} BK{bk} BN{192 if wide else 128}"


def _bits(t):
    return t.view(torch.int16) if t.element_size() == 2 else t.view(torch.int32)


def _filled(shape, dt, dev):
    if dt == torch.float32:
        return torch.full(shape, float("nan"), dtype=dt, device=dev)
    return torch.full(shape, SENTINEL16, dtype=torch.int16, device=dev).view(dt)


def _padded(host, ld, dev):
    """A device view of `host` (rows, K) whose row stride is ld and whose padding columns hold NaN."""
    buf = torch.full((host.shape[0], ld), float("nan"), dtype=host.dtype, device=dev)
    buf[:, :host.shape[1]] = host.to(dev)
    return buf[:, :host.shape[1]]


def _operands(dt, M, N, K, seed, dev):
    g = torch.Generator().manual_seed(seed)
    a_h = torch.randn((M, K), generator=g).to(dt)
    w_h = (torch.randn((N, K), generator=g) / math.sqrt(K)).to(dt)
    bias = torch.randn((N,), generator=g)
    return g, a_h, w_h, bias, _padded(a_h, K + 16, dev), _padded(w_h, K + 24, dev)


def _check(out_h, ref, bnd, what):
    n_bad, worst = G.excess(out_h, ref, bnd)
    rl2 = float((out_h.double() - ref).norm() / ref.norm().clamp_min(1e-300))
    print(f"{what}: rel_l2 {rl2:.2e}, max |err| / bound {worst:.3f}")
    assert n_bad == 0, f"{what}: {n_bad} of {ref.numel()} elements outside the bound (worst {worst:.2f} x)"
    return worst


def _launch_checked(obuf, launch, region, what):
    """Run `launch` on obuf (restored first), check the guard band outside region = (rows, cols), relaunch and compare the bits."""
    before = obuf.clone()
    launch()
    torch.cuda.synchronize()
    after = obuf.clone()
    mask = torch.ones(obuf.shape, dtype=torch.bool, device=obuf.device)
    mask[:region[0], :region[1]] = False
    assert torch.equal(_bits(after)[mask], _bits(before)[mask]), f"{what}: a store outside [M, N]"
    obuf.copy_(before)
    launch()
    assert torch.equal(_bits(obuf), _bits(after)), f"{what}: a second launch gave other bits"
    return after


# (M, N, K, epilogue, gate: None | (rows_per_group, gate_ld - N), ldc - N_out).  M: 1, 63, 65, 127, 129, 257 and 2753 (= 21 x 128 + 65:
# 128-row tiles with a partial last one at N = 3072); N: 16, 13 (scalar stores), 200, 192 k (384, 576), 3072; K: 32 (one k-tile), 96, 512,
# 1056 (long K on 32-deep k-tiles), 2048 (64-deep).  rpg "M": one gate row for the whole call.
CASES = [
    (1, 3072, 2048, S16, None, 8),
    (63, 13, 96, S16, None, 3),
    (65, 200, 1056, GELU, None, 8),
    (127, 384, 32, F32, None, 4),
    (129, 16, 512, RESID, (7, 3), 4),
    (257, 3072, 512, GEGLU, None, 4),
    (2753, 3072, 512, S16, None, 8),
    (257, 576, 1056, RESID, None, 4),
    (65, 13, 2048, RESID, (1, 3), 3),
    (127, 200, 96, RESID, ("M", 4), 4),
    (63, 3072, 32, GELU, None, 8),
    (1, 200, 512, F32, None, 4),
    (129, 384, 2048, GEGLU, None, 8),
    (257, 13, 32, F32, None, 5),
    (2753, 3072, 96, RESID, (7, 4), 4),
    (65, 576, 512, S16, None, 6),                # ldc % 4 != 0: the scalar store path with N % 4 == 0
    (127, 64, 1056, GEGLU, None, 0),
    (1, 13, 1056, GELU, None, 3),
]


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("M,N,K,epi,gate_spec,pad_c", CASES)
def test_four_wave_gemm_elementwise(cuda, dt, M, N, K, epi, gate_spec, pad_c):
    g, a_h, w_h, bias, a, w = _operands(dt, M, N, K, M * 7 + N * 3 + K + epi, cuda)
    n_out = N // 2 if epi == GEGLU else N
    odt = torch.float32 if epi in (F32, RESID) else dt
    obuf = _filled((M + 3, n_out + pad_c), odt, cuda)
    out = obuf[:M, :n_out]
    gate_h = gate = x0 = None
    rpg = gate_ld = 0
    if epi == RESID:
        x0 = torch.randn((M, N), generator=g)
        out.copy_(x0.to(cuda))
        if gate_spec is not None:
            rpg = M if gate_spec[0] == "M" else gate_spec[0]
            gate_ld = N + gate_spec[1]
            gate_h = torch.randn(((M + rpg - 1) // rpg, gate_ld), generator=g)
            gate = gate_h.to(cuda)
    if dit_ops.gemm8_eligible(M, N, K, a.stride(0), w.stride(0), obuf.stride(0), epi) and gate is None:
        assert (M // 256) * (N // 256) < 256                     # the router keeps these on the four-wave kernel
    what = f"{dt} M{M} N{N} K{K} epi{epi} gate{gate_spec} ldc {obuf.stride(0)} [{_variant(M, N, K, epi)}]"
    after = _launch_checked(obuf, lambda: dit_ops.gemm(a, w, bias.to(cuda), out, epi, gate=gate, gate_ld=gate_ld, rows_per_group=rpg),
                            (M, n_out), what)
    ref, bnd = G.model(a_h, w_h, bias, epi, gate=gate_h, rpg=max(rpg, 1), x0=x0)
    _check(after[:M, :n_out].cpu(), ref, bnd, what)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("M,N,K,rpg,gate_pad", [(129, 384, 512, 7, 4), (63, 512, 96, 0, 0), (257, 128, 1056, 1, 8)])
def test_residual_epilogue_row_statistics(cuda, dt, M, N, K, rpg, gate_pad):
    """gvf_gemm_resid_stats: the updated stream within the bound, and the host sum of its gvf_gemm_stats_parts partial (sum, sum of squares)
    pairs against the float64 sums of the updated rows."""
    g, a_h, w_h, bias, a, w = _operands(dt, M, N, K, M + N + K, cuda)
    x0 = torch.randn((M, N), generator=g) + 0.5
    xbuf = _filled((M + 2, N + 4), torch.float32, cuda)
    x = xbuf[:M, :N]
    x.copy_(x0.to(cuda))
    gate_h = torch.randn(((M + rpg - 1) // rpg, N + gate_pad), generator=g) if rpg else None
    gate = None if gate_h is None else gate_h.to(cuda)
    parts = dit_ops.gemm_stats_parts(N)
    assert parts == 2 * ((N + 127) // 128)
    stats = torch.full((M, parts, 2), float("nan"), device=cuda)
    xs = []

    def launch():
        stats.fill_(float("nan"))
        dit_ops.gemm_resid_stats(a, w, bias.to(cuda), x, stats, gate=gate, gate_ld=N + gate_pad, rows_per_group=rpg)
        xs.append(stats.clone())
    after = _launch_checked(xbuf, launch, (M, N), f"{dt} stats M{M} N{N} K{K} rpg{rpg}")
    assert torch.equal(xs[0], xs[1])
    x_h = after[:M, :N].cpu()
    ref, bnd = G.model(a_h, w_h, bias, RESID, gate=gate_h, rpg=max(rpg, 1), x0=x0)
    _check(x_h, ref, bnd, f"{dt} stats M{M} N{N} K{K} stream")
    st = xs[0].cpu().double()
    b_sum, b_sq = G.stats_bound(x_h.view(M, parts, N // parts))
    xd = x_h.double().view(M, parts, N // parts)
    assert bool(((st[..., 0] - xd.sum(-1)).abs() <= b_sum).all()) and bool(((st[..., 1] - (xd * xd).sum(-1)).abs() <= b_sq).all())
    s_all, q_all = st[..., 0].sum(1), st[..., 1].sum(1)
    assert bool(((s_all - x_h.double().sum(1)).abs() <= b_sum.sum(1)).all())
    assert bool(((q_all - (x_h.double() ** 2).sum(1)).abs() <= b_sq.sum(1)).all())


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("M,K,N,epi,affine,adaln_rpg", [(300, 512, 200, S16, True, 0), (256, 1024, 384, GELU, True, 128), (129, 512, 64, F32, False, 256),
                                                         (257, 256, 3072, S16, False, 128)])
def test_layernorm_folded_gemm_against_float64(cuda, dt, M, K, N, epi, affine, adaln_rpg):
    """gemm_resid_stats -> gemm_ln: the projection of the float64 LayerNorm (+ affine, + adaLN of the row group) of the fp32 stream the first
    launch wrote, from the statistics it wrote.  The operand's 16-bit rounding is taken at the float64 value; where the kernel's fp32
    LayerNorm may round to the neighbouring 16-bit value (gemm_ref.ln_operand) the bound widens by that step times |w|."""
    g = torch.Generator().manual_seed(M + K + N)
    Kr = 96
    ar_h = torch.randn((M, Kr), generator=g).to(dt)
    wr_h = (torch.randn((K, Kr), generator=g) / math.sqrt(Kr)).to(dt)
    x0 = 2.0 * torch.randn((M, K), generator=g) + 0.3
    xbuf = _filled((M, K + 8), torch.float32, cuda)
    x = xbuf[:, :K]
    x.copy_(x0.to(cuda))
    parts = dit_ops.gemm_stats_parts(K)
    stats = torch.empty((M, parts, 2), device=cuda)
    dit_ops.gemm_resid_stats(_padded(ar_h, Kr + 8, cuda), _padded(wr_h, Kr + 8, cuda), None, x, stats)
    w_h = (torch.randn((N, K), generator=g) / math.sqrt(K)).to(dt)
    bias = torch.randn((N,), generator=g)
    ln_w, ln_b = (1.0 + 0.2 * torch.randn(K, generator=g), 0.2 * torch.randn(K, generator=g)) if affine else (None, None)
    shift = scale = None
    mod_ld = 0
    if adaln_rpg:
        mod_ld = K + 4
        groups = (M + adaln_rpg - 1) // adaln_rpg
        shift, scale = 0.3 * torch.randn((groups, mod_ld), generator=g), 0.3 * torch.randn((groups, mod_ld), generator=g)
    odt = torch.float32 if epi == F32 else dt
    obuf = _filled((M + 2, N + 8), odt, cuda)
    out = obuf[:M, :N]
    c = lambda t: None if t is None else t.to(cuda)
    w = _padded(w_h, K + 8, cuda)
    after = _launch_checked(obuf, lambda: dit_ops.gemm_ln_bf16(x, stats, parts, w, c(bias), out, epi, eps=1e-6, ln_w=c(ln_w), ln_b=c(ln_b),
                                                               shift=c(shift), scale=c(scale), mod_ld=mod_ld, rows_per_group=adaln_rpg),
                            (M, N), f"{dt} gemm_ln M{M} K{K} N{N}")
    a16, amb = G.ln_operand(x.cpu(), parts, dt, 1e-6, ln_w, ln_b, shift, scale, max(adaln_rpg, 1))
    ref, bnd = G.model(a16, w_h, bias, epi, a_err=amb.abs() @ w_h.double().abs().T)
    _check(after[:M, :N].cpu(), ref, bnd, f"{dt} gemm_ln M{M} K{K} N{N} epi{epi} ({float((amb > 0).double().mean()):.4f} of the operands ambiguous)")


def test_refused_shapes_write_nothing(cuda):
    """Shapes the entry points must refuse return GvfError and leave the output untouched."""
    dt = torch.bfloat16
    g, a_h, w_h, bias, a, w = _operands(dt, 64, 192, 64, 5, cuda)
    obuf = _filled((64, 200), torch.float32, cuda)
    before = obuf.clone()
    with pytest.raises(_lib.GvfError):                      # K % 32 != 0
        dit_ops.gemm(a[:, :48], w[:, :48], None, obuf[:, :192], F32)
    o16 = _filled((64, 64), dt, cuda)
    b16 = o16.clone()
    wg = _padded((torch.randn((96, 64), generator=g)).to(dt), 72, cuda)
    with pytest.raises(_lib.GvfError):                      # GEGLU: N % 64 != 0
        dit_ops.gemm(a, wg, None, o16[:, :48], GEGLU)
    stats = torch.zeros((64, 4, 2), device=cuda)
    with pytest.raises(_lib.GvfError):                      # row statistics: N % 128 != 0
        dit_ops.gemm_resid_stats(a, w, None, obuf[:, :192], stats)
    x = torch.randn((128, 64), device=cuda)
    st = torch.zeros((128, 2, 2), device=cuda)
    sh = torch.zeros((2, 64), device=cuda)
    with pytest.raises(_lib.GvfError):                      # gemm_ln: the adaLN row group must be a multiple of the row tile
        dit_ops.gemm_ln_bf16(x, st, 2, w, None, _filled((128, 192), dt, cuda), S16, shift=sh, scale=sh, mod_ld=64, rows_per_group=100)
    torch.cuda.synchronize()
    assert torch.equal(_bits(obuf), _bits(before)) and torch.equal(_bits(o16), _bits(b16)) and not stats.any()


# ---- row invariance ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("M,N,K,epi,r0,r1", [(12200, 1536, 64, S16, 4000, 4300),     # 128-row / 192-wide tiles (default) vs 64-row ones
                                             (2753, 3072, 512, S16, 65, 194),         # 128-row tiles with a partial last one vs 64-row ones
                                             (2753, 3072, 1056, F32, 1000, 1063),     # long K on 32-deep k-tiles, both tile heights
                                             (2753, 3072, 96, RESID, 700, 1050)])     # gated residual (rpg 7: r0 a group boundary)
def test_four_wave_rows_do_not_depend_on_the_other_rows(cuda, dt, M, N, K, epi, r0, r1):
    """gemm(A)[r0:r1] == gemm(A[r0:r1]) bit for bit although the two calls run other tile shapes (_variant): each output element is one
    fixed chain of MFMA k-steps whatever the tiling."""
    g, a_h, w_h, bias, a, w = _operands(dt, M, N, K, 99 + M + K, cuda)
    bias = bias.to(cuda)
    odt = torch.float32 if epi in (F32, RESID) else dt
    if epi == RESID:
        x0 = torch.randn((M, N), generator=g).to(cuda)
        gate = torch.randn(((M + 6) // 7, N), generator=g).to(cuda)
        full, part = x0.clone(), x0[r0:r1].clone()
        dit_ops.gemm(a, w, bias, full, epi, gate=gate, gate_ld=N, rows_per_group=7)
        dit_ops.gemm(a[r0:r1], w, bias, part, epi, gate=gate[r0 // 7:], gate_ld=N, rows_per_group=7)
    else:
        full = torch.empty((M, N), dtype=odt, device=cuda)
        part = torch.empty((r1 - r0, N), dtype=odt, device=cuda)
        dit_ops.gemm(a, w, bias, full, epi)
        dit_ops.gemm(a[r0:r1], w, bias, part, epi)
    print(f"M{M} [{_variant(M, N, K, epi)}] rows {r0}:{r1} [{_variant(r1 - r0, N, K, epi)}]")
    assert torch.equal(_bits(full[r0:r1]), _bits(part))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("M,N,epi,r0,r1", [(32768, 512, F32, 4096, 8192),        # the static condition projection at batch 8 vs batch 1
                                           (32768, 512, S16, 4096, 8192),
                                           (32768, 512, GEGLU, 4096, 8192),
                                           (12288, 768, RESID, 1920, 3840)])     # gvf_gemm8's 192-wide residual tiles
def test_router_across_the_eight_wave_threshold(cuda, dt, M, N, epi, r0, r1):
    """gvf_gemm sends an eligible call to gvf_gemm8 once it has a tile per CU, so the full call below runs there and its rows r0:r1 alone run on
    the four-wave kernel.  Both kernels chain the 32-deep MFMA k-steps of an element in ascending k and add the bias afterwards: the rows come
    out the same bits either way (measured on the MI355X; include/gvf_dit.h), and both are within the float64 bound.  The full call equals
    gvf_gemm8 called directly; under GVF_GEMM8=0 the router keeps it on the four-wave kernel, which -- the same bits -- the output cannot show."""
    K = 192
    g, a_h, w_h, bias, a, w = _operands(dt, M, N, K, 17 + epi, cuda)
    bias = bias.to(cuda)
    n_out = N // 2 if epi == GEGLU else N
    odt = torch.float32 if epi in (F32, RESID) else dt
    tile = dit_ops.gemm8_eligible(M, N, K, a.stride(0), w.stride(0), n_out, epi)
    assert tile and (M // tile) * (N // tile) >= 256 > ((r1 - r0) // tile) * (N // tile)
    x0 = torch.randn((M, N), generator=g) if epi == RESID else None
    mk = lambda rows: (x0[rows].to(cuda).clone() if epi == RESID else torch.empty((rows.stop - rows.start, n_out), dtype=odt, device=cuda))
    full, part, direct = mk(slice(0, M)), mk(slice(r0, r1)), mk(slice(0, M))
    dit_ops.gemm(a, w, bias, full, epi)
    dit_ops.gemm(a[r0:r1], w, bias, part, epi)
    dit_ops.gemm8(a, w, bias, direct, epi)
    ref, bnd = G.model(a_h[r0:r1], w_h, bias.cpu(), epi, x0=None if x0 is None else x0[r0:r1])
    _check(part.cpu(), ref, bnd, f"{dt} epi{epi} M{r1 - r0} four-wave")
    _check(full[r0:r1].cpu(), ref, bnd, f"{dt} epi{epi} M{M} rows {r0}:{r1} via the router")
    print(f"GVF_GEMM8={os.environ.get('GVF_GEMM8', '1')} epi{epi}: router vs gvf_gemm8 {int((_bits(full) != _bits(direct)).sum())} elements differ, "
          f"rows {r0}:{r1} alone vs in the large call {int((_bits(full[r0:r1]) != _bits(part)).sum())} of {part.numel()}")
    assert torch.equal(_bits(full), _bits(direct))
    assert torch.equal(_bits(full[r0:r1]), _bits(part))


def test_prepare_conditions_does_not_depend_on_the_batch(cuda):
    """DiT.prepare_conditions at the released config (tests/golden/dit_manifest.json): every sample of a batch of 8 -- the batch per rank of
    BASELINE configs[4], where the static condition projection (8 x 4096 x 512 x 192) is large enough for gvf_gemm's eight-wave route -- has
    the same condition products, K / V cache images and position embedding bit for bit as the sample prepared alone."""
    if CHILD:
        pytest.skip("run once, in the parent process")
    from gvfdiffusion_amd.model import dit as dit_mod
    from gvfdiffusion_amd.model.dit import DiT
    man = json.load(open(os.path.join(ROOT, "tests", "golden", "dit_manifest.json")))
    net = DiT(**man["config"])
    net.load_state_dict(synthetic.dit_state_dict(man["state_dict"], seed=0), strict=True)
    net = net.to(cuda).eval()
    B, T = 8, 24
    inp = synthetic.dit_inputs(B=B, T=T, seed=4)
    conds = [inp[k].to(cuda) for k in ("cond_images", "static_latent", "deformation_position_xyz")]
    C, H = net.model_channels, net.num_heads
    Li, Ls = conds[0].shape[2], conds[1].shape[1]
    seen = {}
    real_split3 = dit_ops.split3_bf16

    def spy(src, weights=False, out=None):                 # the fp32 condition products are the inputs of the [hi | lo | hi] expansions
        if not weights and src.shape[1] == C:
            seen["img" if src.shape[0] % (T * Li) == 0 else "st"] = src.clone()
        return real_split3(src, weights, out)

    def run(sl, b):
        seen.clear()
        dit_mod.dit_ops.split3_bf16 = spy
        try:
            net.invalidate_conditions()
            ctx = net.prepare_conditions(conds[0][sl], conds[1][sl], conds[2][sl], T)
        finally:
            dit_mod.dit_ops.split3_bf16 = real_split3
        torch.cuda.synchronize()
        per = lambda t, n_sets_per_sample: t.view(b * n_sets_per_sample, -1)
        return {"img": seen["img"].view(b, -1), "st": seen["st"].view(b, -1),
                "kv_img": [torch.stack([per(k, T), per(v, T)], 1).view(b, -1) for k, v in ctx["kv_img"]],
                "kv_st": [torch.stack([per(k, 1), per(v, 1)], 1).view(b, -1) for k, v in ctx["kv_st"]],
                "pos": ctx["pos"].reshape(b, -1).clone()}

    batch = run(slice(0, B), B)
    batch = {k: ([t.clone() for t in v] if isinstance(v, list) else v) for k, v in batch.items()}
    assert batch["st"].shape == (B, Ls * C) and (B * Ls // 256) * (C // 256) >= 256
    bad = []
    for i in range(B):
        one = run(slice(i, i + 1), 1)
        for name in ("img", "st", "pos"):
            if not torch.equal(one[name][0], batch[name][i]):
                bad.append(f"sample {i} {name}: {int((one[name][0] != batch[name][i]).sum())} elements differ")
        for name in ("kv_img", "kv_st"):
            for blk, (o, bt) in enumerate(zip(one[name], batch[name])):
                if not torch.equal(o[0], bt[i]):
                    bad.append(f"sample {i} {name} block {blk}: {int((o[0] != bt[i]).sum())} bytes differ")
    assert not bad, "\n".join(bad[:20])


def test_variants_forced_in_child_processes(cuda):
    """This file again in three child processes, one at a time, with the tile switches set (read once per process): 128-row and 192-wide tiles
    at every M (GVF_GEMM_BM=128 GVF_GEMM_BN192=2), 64-row tiles with 64-deep k-tiles (GVF_GEMM_BM=64 GVF_GEMM_BK=64), and the large shapes
    kept on the four-wave kernel (GVF_GEMM8=0).  Which tile shape ran does not show in the output bits (that is the row-invariance promise),
    so a child can only assert what the switches select: _variant prints it for every case."""
    if CHILD:
        pytest.skip("the children do not recurse")
    for env in ({"GVF_GEMM_BM": "128", "GVF_GEMM_BN192": "2"}, {"GVF_GEMM_BM": "64", "GVF_GEMM_BK": "64"}, {"GVF_GEMM8": "0"}):
        r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", os.path.abspath(__file__)],
                           cwd=ROOT, env=dict(os.environ, GVF_GEMM_CONFORMANCE_CHILD="1", **env), capture_output=True, text=True, timeout=600)
        print(env, r.stdout.strip().splitlines()[-1] if r.stdout.strip() else "")
        assert r.returncode == 0, f"{env}:\n" + r.stdout[-3000:] + r.stderr[-2000:]
