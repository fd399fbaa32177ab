"""The fp64 reference and error bounds of the row-block launch (tests/rowblock_ref.py) checked on the CPU before any GPU test relies on them:
an fp32 emulation of each stage chain of csrc/rowblock.hip (exact products, fp32 accumulation per 32-deep MFMA k-step, the kernel's epilogue
order, per-wave partial sums of LayerNorm in two different summation orders, round-to-nearest-even 16-bit stores) lies inside the bounds for
bf16 and fp16, and each small bug the bounds exist to catch lands outside them IN THE ROWS OR COLUMNS IT TOUCHES.  Mutants that the
propagated bound of the MLP update cannot see (single 16-bit ulps inside the interior) are kept as tests that say which other check covers
them.  The same stage checkers (rowblock_ref.check_plain / check_mlp / check_hidden_probe) judge the kernel in
tests/test_rowblock_conformance_gpu.py."""
import math

import pytest
import torch

import gemm_ref as G
import rowblock_ref as R
from test_gemm_ref import _truncate16

C, BM = 512, 48
DTYPES = [torch.bfloat16, torch.float16]
F32 = torch.float32


# ---- fp32 emulation of the kernel ---------------------------------------------------------------------------------------------------------

def _r32(x):
    return x.to(F32).double()


def mfma_gemm(a16, w16, acc=None, drop_step=None):
    """acc (fp32 values held as fp64) += a W^T, one fp32 rounding per 32-deep k-step."""
    a, w = a16.double(), w16.double()
    acc = torch.zeros((a.shape[0], w.shape[0]), dtype=torch.float64) if acc is None else acc
    for s in range(a.shape[1] // 32):
        if s != drop_step:
            acc = _r32(acc + a[:, 32 * s:32 * s + 32] @ w[:, 32 * s:32 * s + 32].T)
    return acc


def _store(v32, dt, trunc):
    return _truncate16(v32, dt) if trunc else v32.to(dt)


def _wave_partials(v, order):
    """(M, 512) fp32 -> (M, 8) per-wave sums of 64 columns, in one of two summation orders."""
    p = v.view(-1, 8, 64)
    if order == 0:
        return p.sum(-1)
    s = torch.zeros(p.shape[:2], dtype=F32)
    for i in range(63, -1, -1):
        s = s + p[:, :, i]
    return s


def _seq(p, skip=None):
    tot = torch.zeros(p.shape[0], dtype=F32)
    for w in range(p.shape[1]):
        tot = tot + (p[:, w] if skip is None else torch.where(skip[:, w], torch.zeros(()), p[:, w]))
    return tot


def emu_layernorm(v, d, ln, order=0, mut=None, trunc=False):
    """rb_layernorm on the fp32 rows v -> 16-bit rows.  Mutants act on rows [0, 16) of the second 48-row block (rows 48 .. 63) only."""
    M = v.shape[0]
    rows = torch.arange(M)
    hit = ((rows >= BM) & (rows < BM + 16))[:, None]
    g = rows // d["rpg"]
    one = torch.ones((), dtype=F32)
    w, b, sh, sc = R._ln_args(ln)
    scf = (one + sc[g, :C]) if sc is not None else None
    mul = (w if w is not None else one) * (scf if scf is not None else one)
    add = (b * scf if (b is not None and scf is not None) else (b if b is not None else 0 * one)) + (sh[g, :C] if sh is not None else 0 * one)
    mul, add = mul.expand(M, C), add.expand(M, C)
    if mut == "mul_sum" and sc is not None and w is not None:
        mul = torch.where(hit, (w + sc[g, :C]).expand(M, C), mul)
    if mut == "lnb_unscaled" and sc is not None and b is not None:
        add = torch.where(hit, (b + sh[g, :C]).expand(M, C), add)
    skip = torch.zeros((M, 8), dtype=torch.bool)
    skip[:, 5] = hit[:, 0]
    mean = _seq(_wave_partials(v, order), skip if mut == "mean_partial" else None) * (1.0 / C)
    dd = v - mean[:, None]
    var = _seq(_wave_partials(dd * dd, order), skip if mut == "var_partial" else None) * (1.0 / C)
    if mut == "one_pass":                        # sq / K - mean^2 in place of the centred squares
        var = torch.where(hit[:, 0], _seq(_wave_partials(v * v, order)) * (1.0 / C) - mean * mean, var)
    rstd = torch.rsqrt(var + torch.tensor(d["eps"], dtype=F32))
    if mut == "rstd_tile":                       # rows 48 .. 63 take the rstd of rows 64 .. 79
        rstd = torch.where(hit[:, 0], torch.roll(rstd, -16), rstd)
    y = (dd * rstd[:, None]) * mul + add
    return _store(y, d["dt"], trunc)


def emu_phase1(d, mut=None):
    M, rpg = d["M"], d["rpg"]
    rows = torch.arange(M)
    period = d.get("period", 0) + (1 if mut == "x_in_period" else 0)
    x_in = d.get("x_in")
    if mut == "x_in_period":                     # (the longer period runs past the source: a few more rows for the mutant to read)
        x_in = torch.cat([x_in, x_in[:M // rpg]])
    rs = R.residual_source(d["x0"], x_in, period, rpg).clone()
    if d.get("in_x") is not None:
        if d.get("in_b") is not None and mut != "in_b_dropped":
            rs = rs + d["in_b"]
        for k in range(d["in_x"].shape[1]):
            rs = rs + d["in_x"][:, k:k + 1] * d["in_wt"][k][None]
    if d.get("a") is None:
        return rs
    acc = mfma_gemm(d["a"], d["w1"], drop_step=1 if mut == "drop_w1" else None).to(F32)
    b = d["b1"] if d.get("b1") is not None else torch.zeros(C)
    if mut == "bias_pair":
        b = b[torch.arange(C) & ~1]
    g = rows // rpg
    if mut == "gate_group":                      # the second block reads the first group's gate
        g = torch.where((rows >= BM) & (rows < 2 * BM), g - 1, g)
    gate = d["gate1"][g, :C] if d.get("gate1") is not None else torch.ones((M, C))
    return rs + gate * (acc + b)


def emu_ln_stage(v, d, ln, order, mut, which):
    ln_mut = mut[len(which) + 1:] if mut is not None and mut.startswith(which + ":") else None
    if ln_mut in ("shift_group", "scale_group") and ln.get("scale") is not None:
        key = ln_mut.split("_")[0]
        out = emu_layernorm(v, d, ln, order)
        sw = dict(ln)
        sw[key] = torch.roll(ln[key], 1, 0)      # every group reads its neighbour's row ...
        wrong = emu_layernorm(v, d, sw, order)
        out[BM:2 * BM] = wrong[BM:2 * BM]        # ... in the second block only
        return out
    return emu_layernorm(v, d, ln, order, mut=ln_mut, trunc=ln_mut == "trunc")


def emu_projection(hb, d, mut):
    acc = mfma_gemm(hb, d["w3"], drop_step=7 if mut == "drop_w3" else None).to(F32)
    return _store(acc + (d["b3"] if d.get("b3") is not None else 0.0), d["dt"], mut == "trunc_out3")


def emu_plain(d, order=0, mut=None):
    x = emu_phase1(d, mut)
    hb = emu_ln_stage(x, d, d["ln1"], order, mut, "ln1")
    return x, hb, (emu_projection(hb, d, mut) if d.get("w3") is not None else None)


def emu_gelu(x):
    c0 = torch.tensor(-2.0 * 0.7978845608028654 * 1.4426950408889634, dtype=F32)
    e = torch.exp2(c0 * (x + torch.tensor(0.044715, dtype=F32) * (x * x) * x))
    return x * (1.0 / (1.0 + e))


def emu_mlp(d, order=0, mut=None, zero_gate=False, identity_probe=False):
    M, rpg, dt, hidden = d["M"], d["rpg"], d["dt"], d["hidden"]
    x1 = emu_phase1(d, mut)
    hb = emu_ln_stage(x1, d, d["ln1"], order, mut, "ln1")
    acc2 = torch.zeros((M, C), dtype=torch.float64)
    slices = list(range(hidden // C))
    if mut == "slice_skipped":
        slices.remove(1)
    if mut == "slice_twice":
        slices.insert(1, 1)
    for s in slices:
        sl = slice(C * s, C * s + C)
        acc = mfma_gemm(hb, d["wfc1"][sl], drop_step=3 if (mut == "drop_fc1" and s == 0) else None).to(F32)
        h = emu_gelu(acc + (d["bfc1"][sl] if d.get("bfc1") is not None else 0.0))
        if mut == "gelu_const":
            h = torch.where(torch.arange(M)[:, None] < BM, h, (acc + d["bfc1"][sl]) * torch.sigmoid(1.702 * (acc + d["bfc1"][sl])))
        h16 = _store(h, dt, mut == "trunc_hidden")
        if mut == "hidden_ulp" and s == 0:        # ONE hidden unit of one row one 16-bit step up
            bits = h16.view(torch.int16).clone()
            bits[50, 7] += 1
            h16 = bits.view(dt)
        acc2 = mfma_gemm(h16, d["wfc2"][:, sl], acc2, drop_step=5 if (mut == "drop_fc2" and s == 0) else None)
    g = torch.arange(M) // rpg
    if mut == "gate_m_group":
        g = torch.where((torch.arange(M) >= BM) & (torch.arange(M) < 2 * BM), g - 1, g)
    gate = torch.zeros((M, C)) if zero_gate else (d["gate_m"][g, :C] if d.get("gate_m") is not None else torch.ones((M, C)))
    x = x1 + gate * (acc2.to(F32) + (d["bfc2"] if d.get("bfc2") is not None else 0.0))
    if d.get("w3") is None and not d.get("want_hb"):
        return x1, x, None, None
    hb2 = emu_ln_stage(x, d, d.get("ln2") or {}, order, mut, "ln2")
    return x1, x, hb2, (emu_projection(hb2, d, mut) if d.get("w3") is not None else None)


def _clean(res):
    return {k: int(v[0].sum()) for k, v in res.items() if isinstance(v, tuple)}


# ---- the emulation lies inside the bounds -------------------------------------------------------------------------------------------------

PLAIN = [dict(K1=128, ln1="adaln"), dict(K1=512, ln1="affine", gate1=False, N3=1536), dict(K1=256, ln1="both", b1=False), dict(K1=384, ln1="none", N3=1024),
         dict(K1=0, N3=512, ln1="both", adv=True), dict(K1=0, N3=512, ln1="none", adv=True), dict(M=144, K1=128, ln1="adaln", adv=True),
         dict(K1=0, in_cin=4, x_in=True, period=16), dict(K1=0, in_cin=16, x_in=True, period=48), dict(K1=0, in_cin=8), dict(K1=0, N3=512, ln1="affine")]


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("kw", PLAIN, ids=lambda k: "-".join(f"{a}{b}" for a, b in k.items()))
def test_emulated_plain_launch_is_inside_the_bounds(dt, order, kw):
    d = R.make_case(dt, seed=3, **kw)
    x, hb, out3 = emu_plain(d, order)
    for with_hb in (True, False):
        res = R.check_plain(d, x, hb if with_hb else None, out3)
        assert all(n == 0 for n in _clean(res).values()), (_clean(res), {k: v[1] for k, v in res.items() if isinstance(v, tuple)})
        assert all(torch.isfinite(torch.tensor(v[1])) for v in res.values() if isinstance(v, tuple))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("hidden,N3,ln2,adv", [(2048, 1536, "adaln", False), (512, 512, "both", False), (1024, 0, "none", False), (1536, 1024, "affine", False),
                                               (2048, 512, "adaln", True)])
def test_emulated_mlp_launch_is_inside_the_bounds(dt, order, hidden, N3, ln2, adv):
    d = R.make_case(dt, K1=512, hidden=hidden, N3=N3, ln2=ln2, seed=5, adv=adv)
    x1, x, hb2, out3 = emu_mlp(d, order)
    x1z, xz, _, _ = emu_mlp(d, order, zero_gate=True)
    assert torch.equal(xz, x1z) and torch.equal(x1z, x1)              # a zero gate exposes the phase-1 stream, bit for bit
    for with_hb in (True, False):
        res = R.check_mlp(d, xz, x, hb2 if with_hb else None, out3)
        assert all(n == 0 for n in _clean(res).values()), _clean(res)
    print(f"{dt} hidden {hidden}: median bound of the MLP update {res['x_bound_median']:.2e}, worst |err| / bound {res['x'][1]:.3f}")


@pytest.mark.parametrize("dt", DTYPES)
def test_hidden_unit_probe_exposes_the_hidden_units_exactly(dt):
    d = R.make_probe(dt)
    _, x, _, _ = emu_mlp(d)
    bad, worst = R.check_hidden_probe(d, x)
    assert int(bad.sum()) == 0, (int(bad.sum()), worst)
    assert torch.equal(x.to(dt).float(), x)                            # the stream holds 16-bit values
    pre = (x.double().abs()).flatten()
    assert float(pre.min()) < 1e-3 and float(pre.max()) > 4.0          # the spread the probe is for


# ---- mutants ------------------------------------------------------------------------------------------------------------------------------

def _rows(bad):
    return bad.any(1).nonzero().flatten().tolist()


SECOND_BLOCK = set(range(BM, 2 * BM))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("mut,stage", [("gate_group", "x"), ("ln1:shift_group", "hb"), ("ln1:scale_group", "hb")])
def test_vectors_of_the_neighbouring_group_for_one_block_are_outside_the_bound(dt, mut, stage):
    d = R.make_case(dt, M=144, rpg=48, K1=128, seed=1)
    res = R.check_plain(d, *emu_plain(d, mut=mut))
    rows = set(_rows(res[stage][0]))
    assert rows == SECOND_BLOCK, (stage, sorted(rows))                  # every row of the block, and no other row
    other = [k for k in ("x", "hb", "out3") if k != stage]
    assert all(int(res[k][0].sum()) == 0 for k in other)                # staged checks: the stages behind it follow the kernel's own values


@pytest.mark.parametrize("dt", DTYPES)
def test_bias_of_the_neighbouring_column_is_outside_the_bound(dt):
    d = R.make_case(dt, K1=128, seed=2)
    res = R.check_plain(d, *emu_plain(d, mut="bias_pair"))
    cols = res["x"][0].any(0)
    assert bool(cols[1::2].all()) and not bool(cols[0::2].any())


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("ln1,mut", [("adaln", "mean_partial"), ("both", "mean_partial"), ("adaln", "var_partial"), ("both", "var_partial"),
                                     ("adaln", "rstd_tile"), ("affine", "rstd_tile"), ("both", "mul_sum"), ("both", "lnb_unscaled")])
def test_layernorm_mutants_are_outside_the_bound_in_their_row_tile(dt, ln1, mut):
    d = R.make_case(dt, K1=128, ln1=ln1, seed=4)
    res = R.check_plain(d, *emu_plain(d, mut="ln1:" + mut))
    rows = set(_rows(res["hb"][0]))
    assert rows == set(range(BM, BM + 16)), sorted(rows)                # all 16 rows of the tile, nothing else
    assert int(res["x"][0].sum()) == 0 and int(res["out3"][0].sum()) == 0


@pytest.mark.parametrize("dt", DTYPES)
def test_one_pass_variance_is_outside_the_bound_on_rows_with_a_large_common_offset(dt):
    """var = sq / K - mean^2 loses |mean|^2 / var * 2^-24 of the variance: at |mean| = 1000 sigma every row it acts on (rows 48 .. 63) has
    elements outside the two-pass band, whose own width stays usable there."""
    d = R.make_case(dt, M=96, K1=0, N3=512, ln1="affine", seed=12)
    d["x0"][40:72] += 2000.0
    res = R.check_plain(d, *emu_plain(d))
    assert all(n == 0 for n in _clean(res).values())
    res = R.check_plain(d, *emu_plain(d, mut="ln1:one_pass"))
    assert set(_rows(res["hb"][0])) == set(range(BM, BM + 16))
    assert int(res["x"][0].sum()) == 0 and int(res["out3"][0].sum()) == 0


@pytest.mark.parametrize("dt", DTYPES)
def test_truncating_stores_are_outside_the_bound(dt):
    d = R.make_case(dt, K1=128, seed=6)
    res = R.check_plain(d, *emu_plain(d, mut="ln1:trunc"))
    assert int(res["hb"][0].sum()) > 0.3 * d["M"] * C and int(res["out3"][0].sum()) == 0
    res = R.check_plain(d, *emu_plain(d, mut="trunc_out3"))
    assert int(res["out3"][0].sum()) > 0.3 * d["M"] * C and int(res["hb"][0].sum()) == 0
    # without hb_out the LayerNorm's store is only visible through the projection: a truncated hb moves out3 by about |W3| ulp / 2 per operand,
    # far outside the band of 0.4 % / 2 % ambiguous operands
    x, hb, out3 = emu_plain(d, mut="ln1:trunc")
    res = R.check_plain(d, x, None, out3)
    assert int(res["out3"][0].sum()) > 0.3 * d["M"] * C
    p = R.make_probe(dt)
    bad, _ = R.check_hidden_probe(p, emu_mlp(p, mut="trunc_hidden")[1])
    assert int(bad.sum()) > 0.3 * p["M"] * C
    assert len(set(r // BM for r in _rows(bad))) == p["M"] // BM        # at every magnitude of the probe


@pytest.mark.parametrize("dt", DTYPES)
def test_wrong_gelu_constant_is_outside_the_probe_bound(dt):
    """x sigmoid(1.702 x) in place of the tanh form differs by up to 2e-2: the probe (single-ulp resolution) sees it in every group it acts in."""
    p = R.make_probe(dt)
    bad, _ = R.check_hidden_probe(p, emu_mlp(p, mut="gelu_const")[1])
    rows = set(_rows(bad))
    assert rows and min(rows) >= BM and len(set(r // BM for r in rows)) >= (p["M"] // BM - 1) // 2


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("mut,stage,share", [("drop_w1", "x", 0.9), ("drop_w3", "out3", 0.9), ("drop_fc1", "x", 0.5), ("drop_fc2", "x", 0.8),
                                             ("slice_skipped", "x", 0.95), ("slice_twice", "x", 0.95), ("gate_m_group", "x", None)])
def test_dropped_k_steps_and_slices_are_outside_the_bound(dt, mut, stage, share):
    d = R.make_case(dt, M=144, K1=512, hidden=2048, N3=512, seed=8)
    x1, x, hb2, out3 = emu_mlp(d, mut=mut)
    res = R.check_mlp(d, emu_mlp(d, mut=mut, zero_gate=True)[1], x, hb2, out3)
    if mut == "drop_w1":                                                # phase 1: seen at the zero-gate launch
        stage = "x1"
    bad = res[stage][0]
    if share is None:
        assert set(_rows(bad)) == SECOND_BLOCK
    else:
        assert float(bad.double().mean()) > share, float(bad.double().mean())
    assert all(int(v[0].sum()) == 0 for k, v in res.items() if isinstance(v, tuple) and k != stage)      # every other stage follows the kernel's own values


@pytest.mark.parametrize("dt", DTYPES)
def test_input_layer_mutants_are_outside_the_bound(dt):
    d = R.make_case(dt, M=96, rpg=48, K1=0, in_cin=8, x_in=True, period=16, seed=9)
    for mut in ("x_in_period", "in_b_dropped"):
        res = R.check_plain(d, *emu_plain(d, mut=mut))
        bad = res["x"][0]
        if mut == "in_b_dropped":
            assert float(bad.double().mean()) > 0.99
        else:                                                           # period 17: exactly the rows whose source row differs
            src = lambda r, p: (r // 48) * p + (r % 48) % p
            assert set(_rows(bad)) == {r for r in range(96) if src(r, 17) != src(r, 16)}
        assert int(res["hb"][0].sum()) == 0 and int(res["out3"][0].sum()) == 0


@pytest.mark.parametrize("dt", DTYPES)
def test_single_hidden_ulp_is_inside_the_propagated_bound_and_covered_by_the_probe(dt):
    """One hidden unit one 16-bit step off moves 512 stream elements by |Wfc2| ulp, about 1e-5 .. 1e-4: inside the propagated bound of the MLP
    update wherever the LayerNorm band fans out (documented, not caught here).  The faults that produce such errors systematically -- a
    truncating pack, a wrong GELU constant, a wrong bias column in the hidden stage -- are caught by the hidden-unit probe
    (test_truncating_stores_are_outside_the_bound, test_wrong_gelu_constant_is_outside_the_probe_bound); a one-off single-ulp error of one
    unit in a full launch is covered by no check."""
    d = R.make_case(dt, M=96, K1=512, hidden=2048, N3=0, seed=8)
    x1, x, _, _ = emu_mlp(d, mut="hidden_ulp")
    res = R.check_mlp(d, x1, x)
    assert not torch.equal(x, emu_mlp(d)[1]) and int(res["x"][0].sum()) == 0


@pytest.mark.parametrize("dt", DTYPES)
def test_two_pass_band_is_narrower_than_the_one_pass_band(dt):
    d = R.make_case(dt, K1=128, seed=0)
    x = emu_phase1(d)
    _, amb, _ = R.ln_band(x, dt, 1e-6, *R._ln_args(d["ln1"]), rpg=d["rpg"])
    _, amb1 = G.ln_operand(x, 8, dt, 1e-6, None, None, d["ln1"]["shift"], d["ln1"]["scale"], d["rpg"])
    s2, s1 = R.ambiguous_share(amb), R.ambiguous_share(amb1)
    print(f"{dt}: ambiguous LayerNorm outputs: two-pass band {100 * s2:.3f} %, gemm_ref.ln_operand {100 * s1:.3f} %")
    assert s2 < s1


@pytest.mark.parametrize("dt", DTYPES)
def test_planted_block_error_passes_the_whole_tensor_bars_and_fails_the_bound(dt):
    """What the element-wise bound is for: at M = 12288 one 48-row block whose LayerNorm took the neighbouring group's shift, 2 % off, moves
    rel_l2 of hb by 0.02 / sqrt(256) = 1.3e-3 and one row 10 % off by 9e-4 -- under the 2e-3 / 3e-3 bars of the whole-tensor tests -- and both
    are outside the bound in every row they touch."""
    g = torch.Generator().manual_seed(5)
    M = 12288
    x = torch.randn((M, C), generator=g) * 2 + 0.5
    d = dict(dt=dt, M=M, rpg=M, eps=1e-6, x0=x, ln1={})
    hb = emu_layernorm(x, d, {})
    bad_hb = hb.clone()
    bad_hb[480:528] = (hb[480:528].float() * 1.02).to(dt)
    bad_hb[7000] = (hb[7000].float() * 1.10).to(dt)
    rel_l2 = float((bad_hb.double() - hb.double()).norm() / hb.double().norm())
    assert rel_l2 < 2e-3
    a16, amb, bnd = R.ln_band(x, dt, 1e-6)
    ok, _ = R._stage(hb, a16.double(), bnd)
    bad, _ = R._stage(bad_hb, a16.double(), bnd)
    assert int(ok.sum()) == 0 and set(_rows(bad)) == set(range(480, 528)) | {7000}


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("C", [64, 100, 512, 1028])
@pytest.mark.parametrize("mode", ["affine", "adaln", "both"])
def test_emulated_unfused_layernorm_is_inside_its_band(dt, C, mode):
    """gvf_layernorm_modulate's arithmetic (csrc/elem.hip) in fp32, two summation orders, against ln_band(kernel="elem"); a truncating store
    and a variance of sq / C - mean^2 on rows with a large common offset are outside it."""
    g = torch.Generator().manual_seed(C)
    rows, rpg = 24, 7
    x = torch.randn((rows, C), generator=g) * 2 + 0.5
    x[0:3] += 2000.0                                                     # |mean| = 1000 x std
    x[3] = 3.0
    mod = torch.randn((4, 2 * C), generator=g) * 0.3
    lw, lb = 1 + 0.1 * torch.randn((C,), generator=g), 0.1 * torch.randn((C,), generator=g)
    w, b = (lw, lb) if mode != "adaln" else (None, None)
    sh, sc = (mod[:, :C], mod[:, C:]) if mode != "affine" else (None, None)
    grp = torch.arange(rows) // rpg

    def emu(order, one_pass=False, trunc=False):
        xs = x if order == 0 else x.flip(1)
        cf = torch.tensor(float(C))
        mean = xs.sum(1, keepdim=True) / cf
        dd = x - mean
        var = (dd * dd if order == 0 else (dd * dd).flip(1)).sum(1, keepdim=True) / cf
        if one_pass:
            var = (x * x).sum(1, keepdim=True) / cf - mean * mean
        y = dd * torch.rsqrt(var + torch.tensor(1e-6))
        if w is not None:
            y = y * w + b
        if sc is not None:
            y = y * (1.0 + sc[grp]) + sh[grp]
        return _store(y, dt, trunc)

    a16, amb, bnd = R.ln_band(x, dt, 1e-6, w, b, sh, sc, rpg, kernel="elem")
    for order in (0, 1):
        assert R.excess(emu(order), a16.double(), bnd)[0] == 0
    assert R.excess(emu(0, trunc=True), a16.double(), bnd)[0] > 0.3 * rows * C
    bad = ~((emu(0, one_pass=True).double() - a16.double()).abs() <= bnd)
    assert bool(bad[0:3].any(1).all())                                   # the rows with the large common offset


@pytest.mark.parametrize("dt", DTYPES)
def test_cast_model_holds_the_fp32_silu_and_catches_a_truncating_cast(dt):
    v = torch.cat([torch.randn(4000) * 4, torch.tensor([-200.0, -95.0, -88.0, 90.0, 200.0, 0.0, 1e-5])])
    for act in (0, 1):
        ref, bnd = R.cast_model(v, dt, act)
        f = v if act == 0 else v / (1.0 + torch.exp(-v))
        assert R.excess(f.to(dt), ref, bnd)[0] == 0
        assert R.excess(_truncate16(f, dt), ref, bnd)[0] > 0.3 * v.numel()


# ---- temporal section -------------------------------------------------------------------------------------------------------------------

def emu_temporal(d, order=0, mut=None, zero_gate=False):
    """The temporal launch in fp32 on the token rows (sample, frame, token); padding rows keep the phase-1 stream.  Mutants act on token 1 of
    sample 0 only (the phantom-row one on the last real token)."""
    dt, B, T, N, rpg, M = d["dt"], d["B"], d["T"], d["N"], d["rpg"], d["M"]
    rows = R.token_rows(B, T, N, rpg)
    c = {k: (v[rows] if k in ("x0", "a") else v) for k, v in d.items()}
    c.update(M=rows.numel(), rpg=T * N)
    x1c = emu_phase1(c)
    hb = emu_layernorm(x1c, c, d["ln1"], order)
    Hh = C // 32

    def proj(i):
        acc = mfma_gemm(hb, d["wqkv"][C * i:C * i + C], drop_step=9 if mut == ("drop_wq", "drop_wk", "drop_wv")[i] else None).to(F32)
        pre = acc + (d["bqkv"][C * i:C * i + C] if d.get("bqkv") is not None else 0.0)
        v16 = pre.to(dt).float()
        if mut == ("trunc_q", "trunc_k", "trunc_v")[i]:                                  # ... for the T frames of token 1 of sample 0
            tr = _truncate16(pre, dt).float()
            hit = (torch.arange(B * T * N) % N == 1) & (torch.arange(B * T * N) < T * N)
            v16 = torch.where(hit[:, None], tr, v16)
        return v16.view(B, T, N, Hh, 32).permute(0, 2, 3, 1, 4).contiguous()            # (B, N, H, T, 32)

    q, k, v = proj(0), proj(1), proj(2)

    def rms(t, g):
        ss = (t * t).sum(-1, keepdim=True) if order == 0 else (t * t).flip(-1).sum(-1, keepdim=True)
        inv = math.sqrt(32.0) * torch.rsqrt(torch.clamp_min(ss, 1e-24))
        return (t * inv * g.view(1, 1, Hh, 1, 32)).to(dt).float()

    if d.get("gq") is not None:
        gq, gk = (d["gk"], d["gq"]) if mut == "gains_exchanged" else (d["gq"], d["gk"])
        qn, kn = rms(q, gq), rms(k, gk)
        if mut == "gains_exchanged":                 # ... for token 1 of sample 0
            q0, k0 = rms(q, d["gq"]), rms(k, d["gk"])
            q0[0, 1], k0[0, 1] = qn[0, 1], kn[0, 1]
            qn, kn = q0, k0
        q, k = qn, kn
    cc = torch.tensor(R.c32(d["t_scale"]), dtype=F32)
    s = (q.double() @ k.double().transpose(-1, -2)).to(F32)                                # (B, N, H, T, T)
    vv = v
    if mut == "neighbour_key":                       # token 1 also sees frame 0 of token 2
        s_x = (q[0, 1].double() @ k[0, 2, :, 0:1].double().transpose(-1, -2)).to(F32)       # (H, T, 1)
        s = torch.cat([s, torch.full_like(s[..., :1], float("-inf"))], -1)
        s[0, 1, :, :, T:] = s_x
        vv = torch.cat([v, torch.zeros_like(v[..., :1, :])], -2)
        vv[0, 1, :, T] = v[0, 2, :, 0]
    if mut == "key_dropped" and T > 1:               # token 1 loses its last frame's key
        s[0, 1, :, :, T - 1] = float("-inf")
    if mut == "v_frames_exchanged" and T > 1:
        vv = vv.clone()
        vv[0, 1, :, 0], vv[0, 1, :, 1] = v[0, 1, :, 1], v[0, 1, :, 0]
    m = s.max(-1, keepdim=True).values
    p = torch.exp2(s * cc - m * cc)
    P = p.to(dt).float()
    l = p.sum(-1, keepdim=True) if order == 0 else p.flip(-1).sum(-1, keepdim=True)
    if mut == "l_rounded":
        l2 = P.sum(-1, keepdim=True)
        l = l.clone()
        l[0, 1] = l2[0, 1]
    Pm = P
    if mut == "trunc_P":
        Pm = P.clone()
        Pm[0, 1] = _truncate16(p, dt).float()[0, 1]
    o32 = (Pm.double() @ vv.double()).to(F32) * (1.0 / l)
    o = o32.to(dt)
    if mut == "trunc_o":
        o[0, 1] = _truncate16(o32, dt)[0, 1]
    oc = o.permute(0, 3, 1, 2, 4).reshape(B * T * N, C)
    acc = mfma_gemm(oc, d["wout"], drop_step=4 if mut == "drop_wout" else None).to(F32)
    gate = torch.zeros((rows.numel(), C)) if zero_gate else (d["t_gate"][torch.arange(rows.numel()) // (T * N), :C] if d.get("t_gate") is not None else torch.ones(()))
    xc = x1c + gate * (acc + (d["bout"] if d.get("bout") is not None else 0.0))
    if mut == "phantom_row":                         # frame 0 of the last real token of sample 0 is overwritten with another token's row
        xc = xc.clone()
        xc[N - 1] = xc[N - 2]
    hb2 = emu_layernorm(xc, c, d["t_ln"], order)
    out3c = emu_projection(hb2, c, None)
    x1 = d["x0"].clone()
    x, out3 = d["x0"].clone(), torch.zeros((M, d["w3"].shape[0]), dtype=dt)
    x1[rows], x[rows], out3[rows] = x1c, xc, out3c
    return x1, x, out3


TEMPORAL = [(1, 24, 4), (2, 16, 5), (1, 1, 48), (2, 3, 20), (1, 48, 3), (1, 8, 9)]


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("B,T,N", TEMPORAL)
def test_emulated_temporal_launch_is_inside_the_bounds(dt, order, B, T, N):
    for rms in (True, False):
        d = R.make_temporal(dt, B, T, N, rms=rms, adaln=rms, seed=order)
        x1, x, out3 = emu_temporal(d, order)
        x1z, xz, _ = emu_temporal(d, order, zero_gate=True)
        assert torch.equal(xz, x1z) and torch.equal(x1z, x1)
        res = R.check_temporal(d, xz, x, out3)
        assert all(n == 0 for n in _clean(res).values()), (_clean(res), {k: v[1] for k, v in res.items() if isinstance(v, tuple)})
    print(f"{dt} T{T} N{N}: median bound of the temporal update {res['x_bound_median']:.2e}, worst |err| / bound {res['x'][1]:.3f}")


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("mut", ["neighbour_key", "key_dropped", "v_frames_exchanged", "phantom_row", "drop_wout", "drop_wq", "drop_wk", "drop_wv"])
def test_temporal_mutants_are_outside_the_bound_in_the_rows_they_touch(dt, mut):
    B, T, N = 2, 6, 11                               # 8 tokens per block: the last block of a group holds 3 tokens and 5 phantom ones
    d = R.make_temporal(dt, B, T, N, seed=2)
    x1, x, out3 = emu_temporal(d, mut=mut)
    res = R.check_temporal(d, x1, x, out3)
    bad_rows = set(res["x"][0].any(1).nonzero().flatten().tolist())        # indices into the (sample, frame, token) grid
    if mut in ("drop_wout", "drop_wq", "drop_wk", "drop_wv"):                                  # touch every row: most of them have an element outside
        assert len(bad_rows) > B * T * N // 2
    elif mut == "phantom_row":
        assert bad_rows == {N - 1}
    else:
        touched = {f * N + 1 for f in range(T)}                            # the T frames of token 1 of sample 0
        assert bad_rows and bad_rows <= touched, sorted(bad_rows)
        assert len(bad_rows) >= T // 2, sorted(bad_rows)
    assert int(res["x1"][0].sum()) == 0 and int(res["out3"][0].sum()) == 0


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("mut", ["l_rounded", "gains_exchanged"])
def test_rounding_level_faults_of_the_temporal_interior_are_inside_the_propagated_bound(dt, mut):
    """Inside the propagated bound of a full launch; caught by the attention-output probe instead
    (test_attention_probe_catches_single_ulp_faults_of_the_interior).  l summed from R16(P) instead of the unrounded p moves o by a relative
    2^-9 (bf16) / 2^-12 (fp16) at most and the stream by 5e-3 / 4e-4; gamma_q and gamma_k exchanged leave q . k = sum q^_d k^_d g_q,d g_k,d
    mathematically unchanged and move only the 16-bit roundings of the normalised operands (7e-3 / 1e-3 in the stream).  The worst-case bound
    of the temporal update is far wider than that (median 8.5e-2 / 6.5e-2 on this data: one ambiguous LayerNorm output in 300 makes a tenth of
    q / k / v ambiguous, and the interval method adds their effects linearly through the scores, P, o and |Wout|)."""
    d = R.make_temporal(dt, 2, 6, 11, seed=2)
    x1, x, out3 = emu_temporal(d, mut=mut)
    res = R.check_temporal(d, x1, x, out3)
    assert not torch.equal(x, emu_temporal(d)[1])
    assert int(res["x"][0].sum()) == 0


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("B,T,N", TEMPORAL)
@pytest.mark.parametrize("real_qkv", [False, True])
def test_attention_probe_exposes_the_attention_output(dt, B, T, N, real_qkv):
    for rms in (True, False):
        d = R.make_temporal_probe(dt, B, T, N, rms=rms, real_qkv=real_qkv)
        for order in (0, 1):
            x1, x, _ = emu_temporal(d, order)
            rows = R.token_rows(B, T, N, d["rpg"])
            assert torch.equal(x1, d["x0"])                              # gate1 = 0: the phase-1 stream is x0
            (bad, worst), o_share, ln_share = R.check_attention_probe(d, x)
            assert ln_share == 0.0                                      # the probe's LayerNorm outputs are unambiguous
            assert int(bad.sum()) == 0, (int(bad.sum()), worst)
    print(f"{dt} T{T} N{N} real to_qkv {real_qkv}: attention probe: {100 * o_share:.2f} % of the outputs may hold more than one 16-bit value")


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("mut", ["trunc_o", "trunc_P", "l_rounded", "gains_exchanged", "neighbour_key", "key_dropped", "v_frames_exchanged"])
def test_attention_probe_catches_single_ulp_faults_of_the_interior(dt, mut):
    """At the probe's resolution a truncating pack of o or of P, a denominator summed from the rounded P and exchanged gains (which move only
    the 16-bit roundings of the normalised q and k) are outside the bound in rows of the token they act on (token 1 of sample 0) and nowhere
    else."""
    B, T, N = 2, 6, 11
    d = R.make_temporal_probe(dt, B, T, N)
    (bad, worst), _, _ = R.check_attention_probe(d, emu_temporal(d, mut=mut)[1])
    bad_rows = set(bad.any(1).nonzero().flatten().tolist())
    assert bad_rows and bad_rows <= {f * N + 1 for f in range(T)}, sorted(bad_rows)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("rms", [True, False])
@pytest.mark.parametrize("mut", ["trunc_q", "trunc_k", "trunc_v", "trunc_o"])
def test_attention_probe_with_a_real_projection_catches_truncated_q_k_v(dt, rms, mut):
    """The second form of the probe (a to_qkv of eight random entries per row, so that q, k and v are genuinely rounded): a truncating pack of
    q, of k or of v is outside the bound in every row of the token it acts on (token 1 of sample 0), and nowhere else."""
    B, T, N = 2, 6, 11
    d = R.make_temporal_probe(dt, B, T, N, rms=rms, real_qkv=True)
    (bad, worst), _, _ = R.check_attention_probe(d, emu_temporal(d, mut=mut)[1])
    assert set(bad.any(1).nonzero().flatten().tolist()) == {f * N + 1 for f in range(T)}
