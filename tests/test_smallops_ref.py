"""The fp64 references and bounds of tests/smallops_ref.py checked on the CPU before any GPU test relies on them: a plain fp32 emulation
(one rounding per operation) of each kernel in its own order of operations and in one other legal order (sequential sums and no fused
multiply-add for the dot products and input_layer; the other pairing of the same depth for the LayerNorm sums, whose bound is a depth) lies inside the bound on every case of the GPU matrix that is small enough for the CPU; each small bug the bounds exist to
catch lands outside them in the rows / columns it touches and nowhere else; and the bounds are sharp: in every plain fp32 case no element's
bound reaches 1e-4 of its row's RMS, so a single element moved by that much is caught -- while the same planted error passes the old
whole-tensor bar (rel_l2 < 2e-6).  The same models judge the kernels in tests/test_smallops_conformance_gpu.py."""
import math

import numpy as np
import pytest
import torch

import gemm_ref as G
import smallops_ref as S
from test_gemm_ref import _truncate16

F32, F64 = torch.float32, torch.float64
DTYPES = [torch.bfloat16, torch.float16]
CPU_ROWS = 5000                                                  # cases with more rows are the GPU's grid-wrap cases


def _ids(cases):
    return ["-".join(str(v) for v in c) for c in cases]


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300))


def fma(a, b, c):
    """fl(a b + c): the product of two fp32 values is exact in fp64."""
    return (a.double() * b.double() + c.double()).to(F32)


def tree64(v):
    """(..., 64) fp32 -> (...): the butterfly over the 64 lanes (lane ^ 1, ^ 2, ... ^ 32), one rounding per level."""
    for _ in range(6):
        v = v.view(*v.shape[:-1], v.shape[-1] // 2, 2)
        v = v[..., 0] + v[..., 1]
    return v[..., 0]


def tree64_halves(v):
    """The same sum with the other pairing: lane ^ 32 first, lane ^ 1 last."""
    for _ in range(6):
        h = v.shape[-1] // 2
        v = v[..., h:] + v[..., :h]
    return v[..., 0]


def assert_inside(out, ref, bnd, what):
    n_bad, worst = S.excess(out, ref, bnd)
    assert n_bad == 0, f"{what}: {n_bad} elements of the emulation outside the bound (worst {worst:.3g} x)"
    return worst


def assert_mutant(out, ref, bnd, touched, what):
    """Outside the bound somewhere in `touched` (bool mask of out's shape) and nowhere else."""
    bad = ~((out.double() - ref).abs() <= bnd)
    touched = touched.expand_as(bad)
    assert bool(bad[touched].any()), f"{what}: the mutant is inside the bound everywhere"
    assert not bool(bad[~touched].any()), f"{what}: elements the mutant does not touch are outside the bound"
    return float(bad[touched].double().mean())


# ---- emulations ------------------------------------------------------------------------------------------------------------------------------

def emu_dot(W, v, order=0):
    """out[i][n] = W[n] . v[i] in fp32.  order 0: dot8_f32 / te_dot8 (lane l takes columns 4 l + 256 i .. + 3: products, (a + b) + (c + d), added to
    the lane's sum; the 64-lane tree); order 1: one sequential sum, products rounded."""
    W, v = W.to(F32), v.to(F32)
    N, K = W.shape
    if order == 1:
        acc = torch.zeros((v.shape[0], N), dtype=F32)
        for k in range(K):
            acc = acc + v[:, k:k + 1] * W[:, k][None]
        return acc
    Kp = (K + 255) // 256 * 256
    Wp, vp = torch.zeros((N, Kp), dtype=F32), torch.zeros((v.shape[0], Kp), dtype=F32)
    Wp[:, :K], vp[:, :K] = W, v
    acc = torch.zeros((v.shape[0], N, 64), dtype=F32)
    for i in range(Kp // 256):
        p = vp[:, None, 256 * i:256 * i + 256].reshape(-1, 1, 64, 4) * Wp[None, :, 256 * i:256 * i + 256].reshape(1, N, 64, 4)
        acc = acc + ((p[..., 0] + p[..., 1]) + (p[..., 2] + p[..., 3]))
    return tree64(acc)


def emu_silu(v):
    return v / (1.0 + torch.exp(-v))


def emu_sinusoid(t, F, max_period=10000.0, mut=None):
    half = F // 2
    nlp = S.neg_log_period(max_period)
    j = np.arange(half, dtype=np.float32)
    arg = (nlp * j).astype(np.float32) / np.float32(half - 1 if mut == "half_minus_1" else half)
    f = np.exp(arg.astype(np.float32))
    a = t.numpy().astype(np.float32)[:, None] * f[None]
    c, s = np.cos(a).astype(np.float32), np.sin(a).astype(np.float32)
    return torch.from_numpy(np.concatenate([s, c] if mut == "swap_halves" else [c, s], 1))


def emu_timestep(d, order=0, dt=None, mut=None, trunc=False):
    """-> (t_emb, out) of timestep_embed_f32_kernel (dt None) or timestep_embed_kernel (dt bf16: operands rounded where the kernel rounds)."""
    rnd = (lambda v: v.to(dt).to(F32)) if dt is not None else (lambda v: v)
    zero = torch.zeros(())
    s = rnd(emu_sinusoid(d["t"], d["F"], mut=mut))
    h = emu_dot(d["w0"], s, order) + (d["b0"] if d["b0"] is not None else zero)
    a = rnd(emu_silu(h))
    te = emu_dot(d["w2"], a, order) + (d["b2"] if d["b2"] is not None else zero)
    out = te.clone() if mut == "no_silu2" else emu_silu(te)
    if mut == "last_slice":                                       # the last of the 32 (f32) / 16 (bf16) slices of the second Linear never runs
        per = (d["C"] + (32 if dt is None else 16) - 1) // (32 if dt is None else 16)
        lo = (d["C"] - 1) // per * per
        out[:, lo:] = 0.0
        te[:, lo:] = 0.0
    if dt is not None:
        out = _truncate16(out, dt) if trunc else out.to(dt)
    return te, out


def last_slice_mask(C, n_slices):
    per = (C + n_slices - 1) // n_slices
    m = torch.zeros(C, dtype=torch.bool)
    m[(C - 1) // per * per:] = True
    return m[None]


def emu_input(d, order=0, mut=None):
    x, wt, M, C, Cin = d["x"], d["w_t"], d["M"], d["C"], d["Cin"]
    acc = torch.zeros((M, C), dtype=F32)
    cols = torch.arange(C)
    for k in range(Cin):
        w = wt[k][None]
        if mut == "drop_cin16" and k >= 16:
            continue
        acc = fma(x[:, k:k + 1], w, acc) if order == 0 else acc + x[:, k:k + 1] * w
    b = d["bias"] if d["bias"] is not None else torch.zeros(C)
    if mut == "bias_pair":
        b = b[cols ^ 1]
    if d["pos"] is None:
        out = acc + b
    else:
        rows = torch.arange(M)
        pr = S.pos_rows(M, d["rpg"], d["period"])
        if mut == "pos_group":                                    # the first row of every group but the first reads the group before it
            pr = torch.where((rows % d["rpg"] == 0) & (rows > 0), pr - d["period"], pr)
        p = d["pos"][pr]
        out = p + (acc + b) if order == 0 else (p + acc) + b
    if mut == "drop256":
        out[:, 256:] = 0.0
    return out


def emu_final(d, order=0, mut=None):
    x, M, C, Cout = d["x"], d["M"], d["C"], d["Cout"]
    rows = torch.arange(M)
    fC = torch.tensor(float(C), dtype=F32)
    xp = torch.zeros((M, 512), dtype=F32)
    xp[:, :C] = x
    ok = (torch.arange(512) < C)[None]
    lanes = lambda v: v.view(M, 2, 64, 4)                         # [chunk i][lane][element]: column (64 i + lane) * 4 + e

    def total(v):
        q = lanes(v)
        if order == 1:                                            # the lane's eight values from the right, the tree from the far lanes in
            return tree64_halves((((q[:, 1, :, 3] + q[:, 1, :, 2]) + (q[:, 1, :, 1] + q[:, 1, :, 0])) + (q[:, 0, :, 3] + q[:, 0, :, 2])) + (q[:, 0, :, 1] + q[:, 0, :, 0]))
        return tree64((((q[:, 0, :, 0] + q[:, 0, :, 1]) + (q[:, 0, :, 2] + q[:, 0, :, 3])) + (q[:, 1, :, 0] + q[:, 1, :, 1])) + (q[:, 1, :, 2] + q[:, 1, :, 3]))

    mean = total(xp) / fC
    v = torch.where(ok, xp - mean[:, None], torch.zeros(()))
    var = total(v * v) / fC
    if mut == "one_pass":
        lo, hi = d["adv_rows"]
        one = total(xp * xp) / fC - mean * mean
        var = torch.where((rows >= lo) & (rows < hi), one, var)
    rstd = torch.rsqrt(var + torch.tensor(d["eps"], dtype=F32))
    y = v * rstd[:, None]
    if d["scale"] is not None:
        g = rows // d["rpg"]
        if mut == "group":                                        # the first row of every group but the first reads the group before it
            g = torch.where((rows % d["rpg"] == 0) & (rows > 0), g - 1, g)
        sc, sh = torch.zeros((M, 512)), torch.zeros((M, 512))
        sc[:, :C], sh[:, :C] = d["scale"][g, :C], d["shift"][g, :C]
        y = y * (sc if mut == "scale_no1" else 1.0 + sc) + sh
        y = torch.where(ok, y, torch.zeros(()))
    if mut == "drop256":
        y[:, 256:] = 0.0
    Wp = torch.zeros((Cout, 512), dtype=F32)
    Wp[:, :C] = d["w"]
    if order == 1:
        out = torch.zeros((M, Cout), dtype=F32)
        for c in range(C):
            out = out + y[:, c:c + 1] * Wp[:, c][None]
    else:
        p = lanes(y)[:, None] * Wp.view(1, Cout, 2, 64, 4)         # (M, Cout, 2, 64, 4)
        part = (((p[:, :, 0, :, 0] + p[:, :, 0, :, 1]) + (p[:, :, 0, :, 2] + p[:, :, 0, :, 3])) + (p[:, :, 1, :, 0] + p[:, :, 1, :, 1])) + (p[:, :, 1, :, 2] + p[:, :, 1, :, 3])
        out = tree64(part)
    o = torch.arange(Cout)
    if d["bias"] is not None:
        out = out + (d["bias"][(o ^ 1).clamp_max(Cout - 1)] if mut == "bias_pair" else d["bias"])
    if mut == "swap_o":
        out = out[:, (o ^ 1).clamp_max(Cout - 1)]
    return out


def emu_wave_ln(v, eps, order):
    """wave_layernorm of csrc/vae.hip: lane l sums channels l, l + 64, ... in sequence, the tree, a division by (float)C."""
    M, C = v.shape
    fC = torch.tensor(float(C), dtype=F32)
    ni = (C + 63) // 64

    def total(a):
        ap = torch.zeros((M, ni * 64), dtype=F32)
        ap[:, :C] = a
        ap = ap.view(M, ni, 64)
        acc = torch.zeros((M, 64), dtype=F32)
        for i in (range(ni) if order == 0 else range(ni - 1, -1, -1)):       # order 1: the lane's channels from the top, the tree from the far lanes in
            acc = acc + ap[:, i]
        return tree64(acc) if order == 0 else tree64_halves(acc)

    mean = total(v) / fC
    dd = v - mean[:, None]
    rstd = torch.rsqrt(total(dd * dd) / fC + torch.tensor(eps, dtype=F32))
    return dd * rstd[:, None]


def emu_vae(d, dt, order=0, mut=None, trunc=False):
    """-> (embedding fp32, out 16-bit).  order 1: the other summation order of the LayerNorms (a depth-bounded sum admits no sequential one);
    the Linear is fmaf in the source, in the order of k, and is the same in both."""
    q, W, C, qdim = d["q"], d["W"], d["C"], d["qdim"]
    acc = torch.zeros((d["P"], C), dtype=F32)
    for k in range(qdim):
        acc = fma(q[:, k:k + 1], W[:, k][None], acc)
    e1 = acc + d["b"]
    axis, is_sin, fi = S.point_embed_map(C)
    if mut == "axis_shift":                                       # the (axis, sin | cos) blocks of C / 6 channels shifted by one
        blk = (torch.arange(C) // (C // 6) + 1) % 6
        axis, is_sin = blk // 2, blk % 2 == 0
    ph = q[:, axis] * d["omega"][fi][None]
    e2 = torch.where(is_sin[None], torch.sin(ph), torch.cos(ph))
    eps_e, eps_p = (d["eps_prenorm"], d["eps_embed"]) if mut == "eps_swap" else (d["eps_embed"], d["eps_prenorm"])
    s = emu_wave_ln(e1, eps_e, order) + emu_wave_ln(e2, eps_e, order)
    y = emu_wave_ln(s, eps_p, order)
    return s, (_truncate16(y, dt) if trunc else y.to(dt))


def emu_geglu(x16, order=0, mut=None, trunc=False):
    dt = x16.dtype
    F = x16.shape[1] // 2
    a, g = x16[:, :F].float(), x16[:, F:].float()
    if mut == "halves":
        a, g = g, a
    if mut == "tanh":
        gel = G.gelu_tanh(g.double()).to(F32)
    elif order == 0:
        gel = 0.5 * g * (1.0 + torch.erf(g * 0.70710678118654752440))
    else:
        gel = (0.5 * (1.0 + torch.erf(g * 0.70710678118654752440))) * g
    v = a * gel
    return _truncate16(v, dt) if trunc else v.to(dt)


def f2bf_bits(x):
    """csrc/elem.hip's f2bf on finite fp32 values, in integer arithmetic (numpy uint32)."""
    u = x.numpy().view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) >> 16
    return torch.from_numpy((u & 0xFFFF).astype(np.uint16).view(np.int16).copy())


def emu_split3(x, mode, mut=None):
    Kp = S.pad64(x.shape[1])
    hi_b = f2bf_bits(x)
    hi = hi_b.view(torch.bfloat16)
    diff = x - hi.float()
    lo = _truncate16(diff, torch.bfloat16) if mut == "trunc_lo" else f2bf_bits(diff).view(torch.bfloat16)
    if mut == "layout":
        mode = 1 - mode
    out = torch.zeros((x.shape[0], 3 * Kp), dtype=torch.bfloat16)
    for i, part in enumerate((hi, lo, hi) if mode == 0 else (hi, hi, lo)):
        out[:, i * Kp:i * Kp + x.shape[1]] = part
    return out


# ---- emulations inside ------------------------------------------------------------------------------------------------------------------

def _cpu(cases, rows_at):
    return [c for c in cases if c[rows_at] <= CPU_ROWS]


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("case", _cpu(S.FINAL_CASES, 2), ids=_ids(_cpu(S.FINAL_CASES, 2)))
def test_final_layer_emulation_inside(case, order):
    d = S.make_final(*case)
    ref, bnd = S.final_layer(d["x"], d["w"], d["bias"], d["shift"], d["scale"], d["rpg"], d["eps"])
    print(f"final_layer {case} order {order}: worst |err| / bound {assert_inside(emu_final(d, order), ref, bnd, 'final_layer'):.3f}")


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("case", S.INPUT_CASES, ids=_ids(S.INPUT_CASES))
def test_input_layer_emulation_inside(case, order):
    d = S.make_input(*case)
    ref, bnd = S.input_layer(d["x"], d["w_t"], d["bias"], d["pos"], d["period"], d["rpg"])
    print(f"input_layer {case} order {order}: worst |err| / bound {assert_inside(emu_input(d, order), ref, bnd, 'input_layer'):.3f}")


MOD_CPU = [c for c in S.MODULATION_CASES if c[1] * c[0] <= 4_000_000]


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("case", MOD_CPU, ids=_ids(MOD_CPU))
def test_modulation_emulation_inside(case, order):
    d = S.make_modulation(*case)
    ref, bnd = S.modulation(d["s"], d["w"], d["bias"])
    out = emu_dot(d["w"], d["s"], order) + (d["bias"] if d["bias"] is not None else 0.0)
    print(f"modulation {case} order {order}: worst |err| / bound {assert_inside(out, ref, bnd, 'modulation'):.3f}")


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("case", S.TIMESTEP_F32_CASES, ids=_ids(S.TIMESTEP_F32_CASES))
def test_timestep_f32_emulation_inside(case, order):
    d = S.make_timestep(*case)
    (te, e_te), (out, e_out) = S.timestep_embed_f32(d["t"], d["F"], d["w0"], d["b0"], d["w2"], d["b2"])
    te_e, out_e = emu_timestep(d, order)
    w1, w2 = assert_inside(te_e, te, e_te, "t_emb"), assert_inside(out_e, out, e_out, "silu(t_emb)")
    print(f"timestep_embed_f32 {case} order {order}: worst |err| / bound t_emb {w1:.3f}, out {w2:.3f}")


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("case", S.TIMESTEP_BF16_CASES, ids=_ids(S.TIMESTEP_BF16_CASES))
def test_timestep_bf16_emulation_inside(case, order):
    d = S.make_timestep(*case, dt=torch.bfloat16)
    (te, e_te), (out, e_out) = S.timestep_embed_bf16(d["t"], d["F"], d["w0"], d["b0"], d["w2"], d["b2"])
    te_e, out_e = emu_timestep(d, order, dt=torch.bfloat16)
    w1, w2 = assert_inside(te_e, te, e_te, "t_emb"), assert_inside(out_e, out, e_out, "bf16(silu(t_emb))")
    print(f"timestep_embed_bf16 {case} order {order}: worst |err| / bound t_emb {w1:.3f}, out {w2:.3f}")


VAE_CPU = _cpu(S.VAE_CASES, 2)


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("case", VAE_CPU, ids=_ids(VAE_CPU))
def test_vae_embed_emulation_inside(case, order, dt):
    d = S.make_vae(*case[:4])
    (s, e_s), (y, e_y), amb = S.vae_embed(d["q"], d["W"], d["b"], d["omega"], d["eps_embed"], d["eps_prenorm"], dt)
    s_e, y_e = emu_vae(d, dt, order)
    w1, w2 = assert_inside(s_e, s, e_s, "embedding"), assert_inside(y_e, y, e_y, "16-bit output")
    print(f"vae_embed {case} {dt} order {order}: worst |err| / bound embedding {w1:.3f}, out {w2:.3f}; ambiguous {100 * float((amb > 0).double().mean()):.2f} %")


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("order", [0, 1])
def test_geglu_emulation_inside(order, dt):
    for F, rows in ((8, 1), (264, 777)):
        x = S.make_geglu(F, rows, dt)
        n_bad, worst = S.geglu_check(emu_geglu(x, order), x)
        assert n_bad == 0, f"{n_bad} elements of the emulation outside the bound"
    x = S.make_geglu_all_gates(dt)
    n_bad, worst = S.geglu_check(emu_geglu(x, order), x)
    print(f"geglu all gates {dt} order {order}: worst |err| / bound {worst:.3f}")
    assert n_bad == 0, f"{n_bad} elements of the emulation outside the bound"


SPLIT_CPU = _cpu(S.SPLIT3_CASES, 1)


@pytest.mark.parametrize("case", SPLIT_CPU, ids=_ids(SPLIT_CPU))
def test_split3_reference_equals_the_kernels_integer_rounding(case):
    cols, rows, _, mode = case
    x = S.make_split3(cols, rows)
    x = torch.where(torch.isfinite(x), x, torch.zeros(()))
    assert torch.equal(emu_split3(x, mode).view(torch.int16), S.split3(x, mode).view(torch.int16))


# ---- mutants outside -----------------------------------------------------------------------------------------------------------------------

FINAL_MUT = (512, 14, 40, 16, True, True, True)


@pytest.mark.parametrize("mut", ["group", "bias_pair", "one_pass", "scale_no1", "drop256", "swap_o"])
def test_final_layer_mutants_outside(mut):
    d = S.make_final(*FINAL_MUT)
    ref, bnd = S.final_layer(d["x"], d["w"], d["bias"], d["shift"], d["scale"], d["rpg"], d["eps"])
    rows = torch.arange(d["M"])
    touched = {"group": ((rows % d["rpg"] == 0) & (rows > 0))[:, None], "one_pass": ((rows >= 8) & (rows < 11))[:, None]}.get(mut, torch.ones((1, 1), dtype=torch.bool))
    share = assert_mutant(emu_final(d, 0, mut), ref, bnd, touched.expand(d["M"], d["Cout"]), mut)
    print(f"final_layer mutant {mut}: {100 * share:.0f} % of the touched elements outside")


@pytest.mark.parametrize("mut", ["pos_group", "bias_pair", "drop256", "drop_cin16"])
def test_input_layer_mutants_outside(mut):
    d = S.make_input(512, 24, 1000, (250, 125), True)
    ref, bnd = S.input_layer(d["x"], d["w_t"], d["bias"], d["pos"], d["period"], d["rpg"])
    rows, cols = torch.arange(d["M"])[:, None], torch.arange(d["C"])[None]
    touched = {"pos_group": (rows % 250 == 0) & (rows > 0) & (cols >= 0), "drop256": (cols >= 256) & (rows >= 0)}.get(mut, torch.ones((1, 1), dtype=torch.bool))
    share = assert_mutant(emu_input(d, 0, mut), ref, bnd, touched.expand(d["M"], d["C"]), mut)
    print(f"input_layer mutant {mut}: {100 * share:.0f} % of the touched elements outside")


def test_modulation_mutant_bias_of_the_neighbouring_column():
    d = S.make_modulation(512, 7 * 512 + 3, 2, True)
    ref, bnd = S.modulation(d["s"], d["w"], d["bias"])
    n = torch.arange(d["N"])
    out = emu_dot(d["w"], d["s"]) + d["bias"][(n ^ 1).clamp_max(d["N"] - 1)]
    assert_mutant(out, ref, bnd, torch.ones((1, 1), dtype=torch.bool), "bias_pair")


@pytest.mark.parametrize("mut", ["last_slice", "swap_halves", "half_minus_1", "no_silu2"])
def test_timestep_mutants_outside(mut):
    d = S.make_timestep(256, 512, True, True)
    (te, e_te), (out, e_out) = S.timestep_embed_f32(d["t"], d["F"], d["w0"], d["b0"], d["w2"], d["b2"])
    te_m, out_m = emu_timestep(d, 0, mut=mut)
    B = len(S.T_VALUES)
    touched = last_slice_mask(512, 32).expand(B, 512) if mut == "last_slice" else torch.ones((B, 512), dtype=torch.bool)
    if mut in ("swap_halves", "half_minus_1"):                   # t = 0: cos = 1, sin = 0 whatever the frequency -- only the swap shows there
        touched = touched.clone()
        touched[0] = mut == "swap_halves"
    assert_mutant(out_m, out, e_out, touched, mut)
    if mut != "no_silu2":
        assert_mutant(te_m, te, e_te, touched, mut + " (t_emb)")
    d16 = S.make_timestep(256, 190, True, True, dt=torch.bfloat16)
    (te, e_te), (out, e_out) = S.timestep_embed_bf16(d16["t"], d16["F"], d16["w0"], d16["b0"], d16["w2"], d16["b2"])
    te_m, out_m = emu_timestep(d16, 0, dt=torch.bfloat16, mut=mut)
    touched = last_slice_mask(190, 16).expand(B, 190) if mut == "last_slice" else torch.ones((B, 190), dtype=torch.bool)
    if mut in ("swap_halves", "half_minus_1"):
        touched = touched.clone()
        touched[0] = mut == "swap_halves"
    assert_mutant(out_m, out, e_out, touched, mut + " (bf16)")


def test_truncating_stores_outside():
    everywhere = torch.ones((1, 1), dtype=torch.bool)
    d16 = S.make_timestep(256, 190, True, True, dt=torch.bfloat16)
    (_, _), (out, e_out) = S.timestep_embed_bf16(d16["t"], d16["F"], d16["w0"], d16["b0"], d16["w2"], d16["b2"])
    assert_mutant(emu_timestep(d16, 0, dt=torch.bfloat16, trunc=True)[1], out, e_out, everywhere, "timestep bf16 trunc")
    for dt in DTYPES:
        d = S.make_vae(192, 14, 64, "plain")
        _, (y, e_y), _ = S.vae_embed(d["q"], d["W"], d["b"], d["omega"], d["eps_embed"], d["eps_prenorm"], dt)
        assert_mutant(emu_vae(d, dt, trunc=True)[1], y, e_y, everywhere, f"vae_embed trunc {dt}")
        x = S.make_geglu(264, 777, dt)
        assert S.geglu_check(emu_geglu(x, trunc=True), x)[0] > 0, f"geglu trunc {dt}"
    x = S.make_split3(64, 33)
    ref = S.split3(x, 0)
    mutant = emu_split3(x, 0, "trunc_lo")
    differs = mutant.view(torch.int16) != ref.view(torch.int16)
    assert bool(differs[:, 64:128].any()) and not bool(differs[:, :64].any()) and not bool(differs[:, 128:].any())


def test_split3_layouts_exchanged_outside():
    x = S.make_split3(65, 10)
    for mode in (0, 1):
        differs = emu_split3(x, mode, "layout").view(torch.int16) != S.split3(x, mode).view(torch.int16)
        assert not bool(differs[:, :128].any()) and bool(differs[:, 128:256].any()) and bool(differs[:, 256:].any())


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
def test_vae_embed_mutants_outside(dt):
    everywhere = torch.ones((1, 1), dtype=torch.bool)
    d = S.make_vae(192, 14, 64, "plain")
    (s, e_s), (y, e_y), _ = S.vae_embed(d["q"], d["W"], d["b"], d["omega"], d["eps_embed"], d["eps_prenorm"], dt)
    s_m, y_m = emu_vae(d, dt, mut="axis_shift")
    assert_mutant(s_m, s, e_s, everywhere, "axis_shift (embedding)")
    assert_mutant(y_m, y, e_y, everywhere, "axis_shift")
    d = S.make_vae(192, 14, 65, "tiny")                          # eps decides: var(Linear) = 1e-8 against eps_embed 1e-5 / eps_prenorm 1e-6
    (s, e_s), (y, e_y), _ = S.vae_embed(d["q"], d["W"], d["b"], d["omega"], d["eps_embed"], d["eps_prenorm"], dt)
    s_m, y_m = emu_vae(d, dt, mut="eps_swap")
    assert_mutant(s_m, s, e_s, everywhere, "eps_swap (embedding)")


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("mut", ["tanh", "halves"])
def test_geglu_mutants_outside(mut, dt):
    x = S.make_geglu(264, 777, dt)
    n_bad, _ = S.geglu_check(emu_geglu(x, mut=mut), x)
    print(f"geglu mutant {mut} {dt}: {n_bad} of {777 * 264} elements outside")
    assert n_bad > (0.3 * 777 * 264 if mut == "halves" else 0)


# ---- sharpness ---------------------------------------------------------------------------------------------------------------------------

def _sharp(ref, bnd, what, rows=None):
    """Every element's bound is below 1e-4 of its row's RMS (so that an element moved by that much is outside it), and -- on outputs of at least
    4096 elements -- that single planted error passes the old whole-tensor bar."""
    if rows is not None:
        ref, bnd = ref[rows], bnd[rows]
    rms = ref.pow(2).mean(1, keepdim=True).sqrt()
    ratio = float((bnd / (1e-4 * rms)).max())
    print(f"{what}: largest bound / (1e-4 row RMS) {ratio:.3f}")
    assert ratio < 1.0, f"{what}: a single element moved by 1e-4 of its row's RMS could stay inside the bound ({ratio:.3g})"
    if ref.numel() >= 4096:
        planted = ref.clone()
        r, c = ref.shape[0] // 2, ref.shape[1] // 3
        planted[r, c] += 1e-4 * float(rms[r])
        assert (planted[r, c] - ref[r, c]).abs() > bnd[r, c]
        old = rel_l2(planted, ref)
        assert old < 2e-6, f"{what}: the planted error would have failed the old bar too ({old:.2e})"


def _plain_rows(d):
    keep = torch.ones(d["M"], dtype=torch.bool)
    if d["adv_rows"]:
        keep[d["adv_rows"][0]:d["adv_rows"][1]] = False
    if d.get("scale") is not None and d["adv_rows"]:
        keep[(torch.arange(d["M"]) // d["rpg"]) == (d["M"] - 1) // d["rpg"]] = False      # the group with 1 + scale = 0
    return keep


@pytest.mark.parametrize("case", _cpu(S.FINAL_CASES, 2), ids=_ids(_cpu(S.FINAL_CASES, 2)))
def test_final_layer_bound_is_sharp(case):
    d = S.make_final(*case)
    ref, bnd = S.final_layer(d["x"], d["w"], d["bias"], d["shift"], d["scale"], d["rpg"], d["eps"])
    _sharp(ref, bnd, f"final_layer {case}", _plain_rows(d))


@pytest.mark.parametrize("case", S.INPUT_CASES, ids=_ids(S.INPUT_CASES))
def test_input_layer_bound_is_sharp(case):
    d = S.make_input(*case)
    _sharp(*S.input_layer(d["x"], d["w_t"], d["bias"], d["pos"], d["period"], d["rpg"]), f"input_layer {case}")


@pytest.mark.parametrize("case", MOD_CPU, ids=_ids(MOD_CPU))
def test_modulation_bound_is_sharp(case):
    d = S.make_modulation(*case)
    _sharp(*S.modulation(d["s"], d["w"], d["bias"]), f"modulation {case}")


@pytest.mark.parametrize("case", S.TIMESTEP_F32_CASES, ids=_ids(S.TIMESTEP_F32_CASES))
def test_timestep_f32_bound_is_sharp(case):
    """Stage by stage (smallops_ref.timestep_probe): the sinusoid, the first Linear and its SiLU at |t| <= 1 through W2 = identity; the second
    Linear through W0 = 0; the last SiLU from t_emb itself.  The emulation is inside each probe's bound too.  The chain's own bound (h not
    observable) and the bound at t = 999, 1000 (the phase term) are printed."""
    d = S.make_timestep(*case)
    plain = torch.arange(len(S.T_VALUES)) < S.T_PLAIN
    for kind, rows in (("first", plain), ("second", None)):
        p = S.timestep_probe(d, kind)
        (te, e_te), _ = S.timestep_embed_f32(p["t"], p["F"], p["w0"], p["b0"], p["w2"], p["b2"])
        assert_inside(emu_timestep(p)[0], te, e_te, f"probe {kind}")
        _sharp(te, e_te, f"t_emb probe {kind} {case}", rows)
        if kind == "first":
            rms = te.pow(2).mean(1, keepdim=True).sqrt()
            print(f"  probe first {case}: bound / (1e-4 row RMS) per t {[round(float(v), 3) for v in (e_te / (1e-4 * rms)).max(1).values]}")
    (te, e_te), (out, e_out) = S.timestep_embed_f32(d["t"], d["F"], d["w0"], d["b0"], d["w2"], d["b2"])
    _sharp(*S.silu(te, torch.zeros_like(te)), f"silu(t_emb) from t_emb {case}")
    rms = te.pow(2).mean(1, keepdim=True).sqrt()
    print(f"timestep_embed_f32 {case}: the chain's bound on t_emb is at most {float((e_te / rms)[:S.T_PLAIN].max()):.2e} of the row's RMS at |t| <= 1, "
          f"{float((e_te / rms)[S.T_PLAIN:].max()):.2e} at t = 12.5, 999, 1000 (the phase term)")


VAE_PLAIN = [c for c in VAE_CPU if c[3] not in S.VAE_ADVERSARIAL]


@pytest.mark.parametrize("case", VAE_PLAIN, ids=_ids(VAE_PLAIN))
def test_vae_embed_bound_is_sharp(case):
    """The fp32 embedding as the other fp32 outputs; the 16-bit output by the share of elements whose interval spans more than one 16-bit value: a
    cap on the reference alone, 3 % (bf16) / 12 % (fp16) on the plain cases."""
    d = S.make_vae(*case[:4])
    for dt, cap in ((torch.bfloat16, 0.03), (torch.float16, 0.12)):
        (s, e_s), _, amb = S.vae_embed(d["q"], d["W"], d["b"], d["omega"], d["eps_embed"], d["eps_prenorm"], dt)
        share = float((amb > 0).double().mean())
        print(f"vae_embed {case} {dt}: ambiguous outputs {100 * share:.2f} %")
        assert share <= cap
    _sharp(s, e_s, f"vae embedding {case}")


def test_vae_embed_adversarial_widths_are_reported():
    for case in [c for c in VAE_CPU if c[3] in S.VAE_ADVERSARIAL]:
        d = S.make_vae(*case[:4])
        for dt in DTYPES:
            (s, e_s), _, amb = S.vae_embed(d["q"], d["W"], d["b"], d["omega"], d["eps_embed"], d["eps_prenorm"], dt)
            rms = s.pow(2).mean(1, keepdim=True).sqrt()
            print(f"vae_embed {case} {dt}: ambiguous outputs {100 * float((amb > 0).double().mean()):.2f} %, largest embedding bound {float((e_s / rms).max()):.2e} of the row's RMS")
            assert torch.isfinite(e_s).all()
