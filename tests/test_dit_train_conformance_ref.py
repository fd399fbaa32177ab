"""The fp64 references and bounds of tests/dit_train_bounds.py checked on the CPU before the GPU test relies on them.  A plain fp32 emulation
(one rounding per operation) of every kernel of csrc/dit_train.hip lies inside the bound on every case of the GPU matrix, in the kernel's own
order (lane ownership 4 (lane + 64 i) resp. lane + 64 i, the 64-lane tree, the slot order of the partials and of the finaliser) and in
another legal one (every lane sum in sequence and from the other end, the other pairing of every tree, waves and slots from the top); each
small bug the bounds exist to catch lands outside them in the elements it touches and nowhere else; a single element moved by twice its own
bound is flagged by the element-wise check and passes the relative-L2 bar of tests/test_dit_train_ops_gpu.py; and the share of 16-bit outputs
whose interval spans more than one value stays under 5 % on plain inputs."""
import functools

import numpy as np
import pytest
import torch

import dit_train_bounds as B
import dit_train_ref as R
import rowblock_ref as RB
from test_dit_train_ops_gpu import _check
from test_gemm_ref import _truncate16

F32 = torch.float32
DTYPES = [torch.bfloat16, torch.float16]
DT_IDS = ["bf16", "fp16"]
SQRT32_F = torch.tensor(5.656854249492381, dtype=F32)


def _ids(cases):
    return ["-".join(str(v) for v in c) for c in cases]


# ---- emulation: sums ---------------------------------------------------------------------------------------------------------------------------

def tree(v, order):
    """(..., n) fp32, n a power of two -> (...): the exchange butterfly, one rounding per level.  order 0: lane ^ 1 first (the kernels'); order 1:
    the far half first."""
    while v.shape[-1] > 1:
        if order == 0:
            v = v.view(*v.shape[:-1], v.shape[-1] // 2, 2)
            v = v[..., 0] + v[..., 1]
        else:
            h = v.shape[-1] // 2
            v = v[..., h:] + v[..., :h]
    return v[..., 0]


def lanes(t, C):
    """(rows, C) -> (rows, n_i, 64, per): element [i][lane][e] is column 4 (lane + 64 i) + e (vector kernels) resp. lane + 64 i (generic)."""
    rows = t.shape[0]
    if B.vec_path(C):
        return t.view(rows, C // 256, 64, 4)
    n = (C + 63) // 64
    p = torch.zeros((rows, n * 64), dtype=F32)                     # the columns past C are not added by the kernel; + 0 is exact
    p[:, :C] = t
    return p.view(rows, n, 64, 1)


def row_sum(t, C, order, paired):
    """Sum over the columns of each row as a wave of the kernels does it.  paired: (a + b) + (c + d) of a lane's float4, added to its sum."""
    q = lanes(t, C)
    s = torch.zeros((t.shape[0], 64), dtype=F32)
    n_i, per = q.shape[1], q.shape[3]
    if order == 0 and paired and per == 4:
        for i in range(n_i):
            s = s + ((q[:, i, :, 0] + q[:, i, :, 1]) + (q[:, i, :, 2] + q[:, i, :, 3]))
        return tree(s, 0)
    idx = [(i, e) for i in range(n_i) for e in range(per)]
    for i, e in (idx if order == 0 else reversed(idx)):
        s = s + q[:, i, :, e]
    return tree(s, order)


@functools.lru_cache(maxsize=None)
def row_layout(rows, rpg, vec, per_group):
    """For every row: the slot its workgroup's partial goes to, the wave that adds it and its position in that wave's sequence."""
    slot, wave, pos = np.zeros(rows, np.int64), np.zeros(rows, np.int64), np.zeros(rows, np.int64)
    seen = {}
    for wg, g, s0, s1 in B.segments(rows, rpg):
        for r in range(s0, s1):
            sl = wg + g if per_group else wg
            wv = (r - s0) % 4 if vec else 0
            slot[r], wave[r], pos[r] = sl, wv, seen.get((sl, wv), 0)
            seen[(sl, wv)] = pos[r] + 1
    count = np.array([seen[(s, w)] for s, w in zip(slot, wave)], np.int64)
    W = (rows + B.RPW - 1) // B.RPW
    return torch.from_numpy(slot), torch.from_numpy(wave), torch.from_numpy(pos), torch.from_numpy(count), W + ((rows + rpg - 1) // rpg if per_group else 0)


def emu_partials(t, rows, rpg, vec, per_group, order=0, mut=None):
    """The workspace after the main launch: (n_slots, cols) fp32, NaN where no workgroup wrote."""
    slot, wave, pos, count, n_slots = row_layout(rows, rpg, vec, per_group)
    if order == 1:
        pos = count - 1 - pos
    acc = torch.zeros((n_slots, 4, t.shape[1]), dtype=F32)
    for p in range(int(pos.max()) + 1):
        sel = pos == p
        acc[slot[sel], wave[sel]] = acc[slot[sel], wave[sel]] + t[sel]
    if mut == "drop_wave3":
        comb = (acc[:, 0] + acc[:, 1]) + acc[:, 2]
    elif order == 0:
        comb = ((acc[:, 0] + acc[:, 1]) + acc[:, 2]) + acc[:, 3]
    else:
        comb = ((acc[:, 3] + acc[:, 2]) + acc[:, 1]) + acc[:, 0]
    out = torch.full((n_slots, t.shape[1]), float("nan"), dtype=F32)
    written = torch.zeros(n_slots, dtype=torch.bool)
    written[slot] = True
    out[written] = comb[written]
    return out


def emu_finalize(part, rows, rpg, factor=None, order=0, mut=None):
    """colsum_finalize_kernel: thread k of a column adds slots lo + k, lo + k + 4, ... of group g; (0 + 1) + (2 + 3); * factor."""
    lo, hi = B.group_slots(rows, rpg)
    if mut == "drop_last_slot":
        hi = hi - 1                                               # for (w = lo + k; w < hi; w += 4)
    G = len(lo)
    gs, ks, ps, ws = [], [], [], []
    for g in range(G):
        n = int(hi[g] - lo[g] + 1)
        for j in range(n):
            k, p = j % 4, j // 4
            if order == 1:
                p = (n - k + 3) // 4 - 1 - p                      # each thread's slots from the top
            gs.append(g), ks.append(k), ps.append(p), ws.append(int(lo[g]) + j)
    gs, ks, ps, ws = (torch.tensor(v, dtype=torch.int64) for v in (gs, ks, ps, ws))
    red = torch.zeros((G, 4, part.shape[1]), dtype=F32)
    for p in range(int(ps.max()) + 1 if len(ps) else 0):
        sel = ps == p
        red[gs[sel], ks[sel]] = red[gs[sel], ks[sel]] + part[ws[sel]]
    out = (red[:, 0] + red[:, 1]) + (red[:, 2] + red[:, 3]) if order == 0 else (red[:, 0] + red[:, 2]) + (red[:, 1] + red[:, 3])
    return out if factor is None else out * factor


def emu_colsum(t, rows, rpg, vec, per_group, factor=None, order=0, mut=None):
    part = emu_partials(t, rows, rpg, vec, per_group, order, mut)
    return emu_finalize(part, rows, rpg if per_group else rows, factor, order, mut)


# ---- emulation: the kernels ------------------------------------------------------------------------------------------------------------------

def _group_index(rows, rpg, mut):
    r = torch.arange(rows)
    g = r // rpg
    if mut == "prev_group":                                       # the first row of every group but the first reads the group before it
        g = torch.where((r % rpg == 0) & (r > 0), g - 1, g)
    return g


def emu_ln(d, dres=None, w=None, b=None, scale=None, rpg=None, eps=1e-6, order=0, mut=None):
    """ln_bwd_kernel<VPL> / ln_bwd_generic_kernel + the finaliser.  -> dict dx, dx_nodres, and the column sums of the call."""
    x, dy = d["x"], d["dy"].float()
    rows, C = x.shape
    vec = B.vec_path(C)
    fC = torch.tensor(float(C), dtype=F32)
    mean = row_sum(x, C, order, True) / fC
    cen = x - mean[:, None]
    mean_lo = row_sum(cen, C, order, True) / fC
    if mut == "one_term_mean":
        mean_lo[0:3] = 0.0                                        # on the rows whose mean is 100 x their spread
    v = cen - mean_lo[:, None]
    rstd = torch.rsqrt(row_sum(v * v, C, order, True) / fC + torch.tensor(eps, dtype=F32))
    xh = v * rstd[:, None]
    if scale is not None:
        m = 1.0 + scale[_group_index(rows, rpg, mut)]
        gm = dy * m
    else:
        gm = dy
    g = gm * w if w is not None else gm
    c1 = row_sum(g, C, order, False) / fC
    c2 = row_sum((dy if mut == "c2_from_dy" else g) * xh, C, order, False) / fC
    t = rstd[:, None] * ((g - c1[:, None]) - xh * c2[:, None])
    out = {"dx_nodres": t, "dx": d["dres"] + t if dres is not None else t}
    if scale is not None:
        a = xh * w + b if w is not None else xh
        out["dshift"] = emu_colsum(dy, rows, rpg, vec, True, None, order, mut)
        out["dscale"] = emu_colsum(dy * a, rows, rpg, vec, True, None, order, mut)
    if w is not None:
        seg = rpg if scale is not None else rows
        out["dw"] = emu_colsum(gm * xh, rows, seg, vec, False, None, order, mut)
        out["db"] = emu_colsum(gm, rows, seg, vec, False, None, order, mut)
    return out


def emu_gate(d, gated, dt, order=0, mut=None):
    x, h, dout = d["x"], d["h"].float(), d["dout"]
    rows, C = x.shape
    store = (lambda t: _truncate16(t, dt)) if mut == "trunc" else (lambda t: t.to(dt))
    if not gated:
        return {"out": x + h, "dh": store(dout)}
    gt = d["gate"][_group_index(rows, d["rpg"], mut)]
    return {"out": x + gt * h, "dh": store(gt * dout),
            "dgate": emu_colsum(dout * h, rows, d["rpg"], B.vec_path(C), True, None, order, mut)}


def emu_rms(d, dt, order=0, mut=None):
    """rms_fwd_kernel / rms_bwd_kernel + the finaliser: a lane holds 8 consecutive channels, d / 8 lanes a head."""
    rows, H, D = d["x"].shape
    NL = D // 8
    f = d["x"].float().view(rows, H, NL, 8)
    dy = d["dy"].float().view(rows, H, NL, 8)
    gm = d["gamma"].view(1, H, NL, 8)
    sqrt_d = SQRT32_F if D == 32 else torch.tensor(8.0, dtype=F32)
    seq = range(8) if order == 0 else range(7, -1, -1)

    def head_sum(lane_vals):                                      # (rows, H, NL) -> (rows, H, NL, 1): what every lane of the head holds
        if mut == "four_lanes" and NL == 8:                       # group_sum<4> on a d = 64 head: each half of the head on its own
            s = tree(lane_vals.view(rows, H, 2, 4), order)
            return s[..., None].expand(rows, H, 2, 4).reshape(rows, H, NL, 1)
        return tree(lane_vals, order)[..., None, None].expand(rows, H, NL, 1)

    ss = torch.zeros((rows, H, NL), dtype=F32)
    for e in seq:
        ss = ss + f[..., e] * f[..., e]
    den = torch.sqrt(head_sum(ss)).clamp_min(torch.tensor(1e-12, dtype=F32))
    xt = f / den
    y = (xt * gm) * sqrt_d
    u = (dy * gm) * sqrt_d
    dl = torch.zeros((rows, H, NL), dtype=F32)
    for e in seq:
        dl = dl + u[..., e] * xt[..., e]
    o = (u - xt * head_sum(dl)) / den
    store = (lambda t: _truncate16(t, dt)) if mut == "trunc" else (lambda t: t.to(dt))
    dgamma = emu_colsum((dy * xt).reshape(rows, H * D), rows, rows, True, False, None if mut == "no_sqrt_d" else sqrt_d, order,
                        mut if mut == "drop_last_slot" else None)
    return {"y": store(y.reshape(rows, H, D)), "dx": store(o.reshape(rows, H, D)), "dgamma": dgamma}


# ---- checks ----------------------------------------------------------------------------------------------------------------------------------

def outside(out, model, dt=None):
    """bool mask of the elements of `out` outside the bound of model = (ref, bound) | (ref, E, bound)."""
    ref = model[0]
    o = out.double().reshape(ref.shape)
    if len(model) == 3:
        return ~((o >= B.r16(ref - model[1], dt)) & (o <= B.r16(ref + model[1], dt)))
    return ~((o - ref).abs() <= model[1])


def inside(out, model, what, dt=None):
    if len(model) == 3:
        n_bad, worst = B.check16(out, model[0], model[1], dt)
    else:
        n_bad, worst = B.excess(out.double().reshape(model[0].shape), model[0], model[1])
    assert n_bad == 0, f"{what}: {n_bad} elements of the emulation outside the bound (worst {worst:.3g} x)"
    return worst


def assert_mutant(out, model, touched, what, dt=None, required=True):
    """Outside the bound somewhere in `touched` (required) and nowhere else."""
    bad = outside(out, model, dt)
    touched = touched.expand_as(bad) if touched.dim() == bad.dim() else touched.reshape(-1, *([1] * (bad.dim() - 1))).expand_as(bad)
    assert not bool(bad[~touched].any()), f"{what}: elements the mutant does not touch are outside the bound"
    if required:
        assert bool(bad[touched].any()), f"{what}: the mutant is inside the bound everywhere"
    return float(bad[touched].double().mean()) if bool(touched.any()) else 0.0


ALL = torch.ones((1, 1), dtype=torch.bool)
NONE = torch.zeros((1, 1), dtype=torch.bool)


# ---- emulations inside -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("mode", B.MODES)
@pytest.mark.parametrize("case", B.LN_CASES, ids=_ids(B.LN_CASES))
def test_layernorm_backward_emulation_inside(case, mode, dt, order):
    d = B.make_ln(*case, dt)
    log = []
    for with_dres in (True, False):
        kw = B.ln_args(d, mode, with_dres)
        model = B.ln_bwd(d["x"], d["dy"], **kw)
        emu = emu_ln(d, order=order, **kw)
        for name, mb in model.items():
            log.append(f"{name} {inside(emu[name], mb, f'{case} {mode} {name}'):.3f}")
            assert torch.isfinite(mb[1]).all()
    print(f"ln_bwd {case} {mode} {dt} order {order}: worst |err| / bound", "; ".join(log))


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("gated", [True, False], ids=["gate", "nogate"])
@pytest.mark.parametrize("case", B.LN_CASES, ids=_ids(B.LN_CASES))
def test_gate_emulation_inside(case, gated, dt, order):
    d = B.make_gate(*case, dt)
    model = B.gate_fwd_bwd(d["x"], d["h"], d["dout"], d["gate"] if gated else None, d["rpg"], dt)
    emu = emu_gate(d, gated, dt, order)
    log = [f"{name} {inside(emu[name], mb, f'{case} {name}'):.3f}" for name, mb in model.items()]
    print(f"gate {case} {'gate' if gated else 'nogate'} {dt} order {order}: worst |err| / bound", "; ".join(log))


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("case", B.RMS_CASES, ids=_ids(B.RMS_CASES))
def test_rmsnorm_emulation_inside(case, dt, order):
    d = B.make_rms(*case, dt)
    model = B.rms_fwd_bwd(d["x"], d["dy"], d["gamma"], dt)
    emu = emu_rms(d, dt, order)
    log = [f"{name} {inside(emu[name], mb, f'{case} {name}', dt):.3f}" for name, mb in model.items()]      # no row exempt: the emulation holds u / 1e-12 too
    print(f"rms {case} {dt} order {order}: worst |err| / bound", "; ".join(log))


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_rmsnorm_forward_count_agrees_with_rowblock_ref(dt):
    """rowblock_ref._rms16 models the same normalisation for the row-block kernel (d = 32, the hardware rsq: 11 U |a|).  On exactly known
    operands both give the same correctly rounded value, and this kernel's count (a correctly rounded sqrtf and division: 10.5 U |a|) is
    the narrower of the two by half a rounding, no more."""
    r = B.make_rms(130, 16, 32, dt, plain=True)
    ref, E, _ = B.rms_fwd_bwd(r["x"], r["dy"], r["gamma"], dt)["y"]
    x = r["x"].double().reshape(1, 130, 16, 1, 32)
    c, amb = RB._rms16(x, torch.zeros_like(x), r["gamma"], dt)
    assert torch.equal(B.r16(ref, dt), c.reshape(ref.shape))
    e_rb = 11.0 * B.U32 * ref.abs()
    assert bool((E <= e_rb).all()) and bool((E >= (10.0 / 11.0) * e_rb).all())


def test_slot_layout_matches_the_header():
    """Every slot the finaliser reads was written by exactly the workgroups of its group, the slots of a group are consecutive, and the
    workspace of W + G slots holds them (include/gvf_dit_train.h)."""
    for C, rows, rpg in B.LN_CASES + [(256, 64, 16), (256, 48, 5)]:
        lo, hi = B.group_slots(rows, rpg)
        W, G = (rows + B.RPW - 1) // B.RPW, (rows + rpg - 1) // rpg
        want = {}
        for wg, g, s0, s1 in B.segments(rows, rpg):
            want.setdefault(g, []).append(wg + g)
        for g in range(G):
            assert want[g] == list(range(int(lo[g]), int(hi[g]) + 1)), (rows, rpg, g)
        assert int(hi[-1]) < W + G
        assert all(int(lo[g + 1]) > int(hi[g]) for g in range(G - 1))


# ---- mutants outside ---------------------------------------------------------------------------------------------------------------------------

def _first_rows(rows, rpg):
    r = torch.arange(rows)
    return (r % rpg == 0) & (r > 0)


def _wave3_groups(rows, rpg):
    """(groups with a segment of at least 4 rows: wave 3 adds a row to their partial, any such segment at all)."""
    G = (rows + rpg - 1) // rpg
    hit = torch.zeros(G, dtype=torch.bool)
    for wg, g, s0, s1 in B.segments(rows, rpg):
        if s1 - s0 >= 4:
            hit[g] = True
    return hit


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_one_term_mean_outside(dt):
    """Dropping mean_lo on the three rows with a +200 offset: where a group is one row (rows_per_group = 1), dscale of that group IS dy * xh of that
    row and the half ulp of the mean in xh shows; dx and the sums over many rows may hide it and are only held to 'nowhere else'."""
    d = B.make_ln(256, 1100, 1, dt)
    kw = B.ln_args(d, "both", True)
    model = B.ln_bwd(d["x"], d["dy"], **kw)
    emu = emu_ln(d, mut="one_term_mean", **kw)
    rows3 = torch.arange(1100) < 3
    share = assert_mutant(emu["dscale"], model["dscale"], rows3, "dscale")
    assert_mutant(emu["dx"], model["dx"], rows3, "dx", required=False)
    assert_mutant(emu["dshift"], model["dshift"], NONE, "dshift", required=False)
    for name in ("dw", "db"):
        assert_mutant(emu[name], model[name], ALL, name, required=False)
    print(f"one-term mean {dt}: {100 * share:.0f} % of dscale of the three rows outside")


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("case", [(768, 50, 7), (100, 163, 81)], ids=_ids([(768, 50, 7), (100, 163, 81)]))
def test_previous_groups_scale_or_gate_outside(case, dt):
    C, rows, rpg = case
    d = B.make_ln(*case, dt)
    kw = B.ln_args(d, "both", True)
    model = B.ln_bwd(d["x"], d["dy"], **kw)
    emu = emu_ln(d, mut="prev_group", **kw)
    first = _first_rows(rows, rpg)
    assert_mutant(emu["dx"], model["dx"], first, "dx")
    for name in ("dshift", "dscale"):                             # they do not read the scale
        assert_mutant(emu[name], model[name], NONE, name, required=False)
    for name in ("dw", "db"):
        assert_mutant(emu[name], model[name], ALL, name)
    g = B.make_gate(*case, dt)
    model = B.gate_fwd_bwd(g["x"], g["h"], g["dout"], g["gate"], rpg, dt)
    emu = emu_gate(g, True, dt, mut="prev_group")
    assert_mutant(emu["out"], model["out"], first, "out")
    assert_mutant(emu["dh"], model["dh"], first, "dh", dt)
    assert_mutant(emu["dgate"], model["dgate"], NONE, "dgate", required=False)


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("case", [(512, 163, 81), (256, 1100, 1), (100, 163, 81)], ids=_ids([(512, 163, 81), (256, 1100, 1), (100, 163, 81)]))
def test_finaliser_dropping_the_last_slot_outside(case, dt):
    C, rows, rpg = case
    d = B.make_ln(*case, dt)
    kw = B.ln_args(d, "both", True)
    model = B.ln_bwd(d["x"], d["dy"], **kw)
    emu = emu_ln(d, mut="drop_last_slot", **kw)
    assert_mutant(emu["dx"], model["dx"], NONE, "dx", required=False)
    for name in ("dshift", "dscale", "dw", "db"):
        assert_mutant(emu[name], model[name], ALL, name)
    g = B.make_gate(*case, dt)
    model = B.gate_fwd_bwd(g["x"], g["h"], g["dout"], g["gate"], rpg, dt)
    emu = emu_gate(g, True, dt, mut="drop_last_slot")
    assert_mutant(emu["dgate"], model["dgate"], ALL, "dgate")
    assert_mutant(emu["dh"], model["dh"], NONE, "dh", dt, required=False)
    r = B.make_rms(41, 12, 64, dt)
    model = B.rms_fwd_bwd(r["x"], r["dy"], r["gamma"], dt)
    assert_mutant(emu_rms(r, dt, mut="drop_last_slot")["dgamma"], model["dgamma"], ALL, "dgamma")


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("case", [(768, 50, 7), (512, 163, 81), (256, 1100, 1)], ids=_ids([(768, 50, 7), (512, 163, 81), (256, 1100, 1)]))
def test_fourth_wave_dropped_in_flush_cols_outside(case, dt):
    """Touched: the groups with a segment of at least four rows (only then has wave 3 a row).  With one row per group every row goes to wave 0
    and the mutant touches nothing: it must then be inside everywhere."""
    C, rows, rpg = case
    d = B.make_ln(*case, dt)
    kw = B.ln_args(d, "both", True)
    model = B.ln_bwd(d["x"], d["dy"], **kw)
    emu = emu_ln(d, mut="drop_wave3", **kw)
    hit = _wave3_groups(rows, rpg)
    for name in ("dshift", "dscale"):
        assert_mutant(emu[name], model[name], hit, name, required=bool(hit.any()))
    for name in ("dw", "db"):
        assert_mutant(emu[name], model[name], ALL if bool(hit.any()) else NONE, name, required=bool(hit.any()))
    assert_mutant(emu["dx"], model["dx"], NONE, "dx", required=False)
    g = B.make_gate(*case, dt)
    model = B.gate_fwd_bwd(g["x"], g["h"], g["dout"], g["gate"], rpg, dt)
    assert_mutant(emu_gate(g, True, dt, mut="drop_wave3")["dgate"], model["dgate"], hit, "dgate", required=bool(hit.any()))


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_head_sum_over_four_lanes_outside(dt):
    r = B.make_rms(41, 12, 64, dt, plain=True)
    model = B.rms_fwd_bwd(r["x"], r["dy"], r["gamma"], dt)
    emu = emu_rms(r, dt, mut="four_lanes")
    for name in ("y", "dx", "dgamma"):
        share = assert_mutant(emu[name], model[name], ALL, name, dt)
        print(f"four-lane head sum {dt} {name}: {100 * share:.0f} % outside")
    r = B.make_rms(37, 2, 32, dt, plain=True)                    # a d = 32 head IS four lanes: untouched
    model = B.rms_fwd_bwd(r["x"], r["dy"], r["gamma"], dt)
    emu = emu_rms(r, dt, mut="four_lanes")
    for name in ("y", "dx", "dgamma"):
        assert_mutant(emu[name], model[name], NONE, name, dt, required=False)


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_truncating_stores_outside(dt):
    g = B.make_gate(768, 50, 7, dt, plain=True)
    for gated in (True, False):
        model = B.gate_fwd_bwd(g["x"], g["h"], g["dout"], g["gate"] if gated else None, 7, dt)
        emu = emu_gate(g, gated, dt, mut="trunc")
        assert_mutant(emu["dh"], model["dh"], ALL, "dh", dt)
        assert_mutant(emu["out"], model["out"], NONE, "out", required=False)
        if gated:
            assert_mutant(emu["dgate"], model["dgate"], NONE, "dgate", required=False)
    r = B.make_rms(41, 12, 64, dt, plain=True)
    model = B.rms_fwd_bwd(r["x"], r["dy"], r["gamma"], dt)
    emu = emu_rms(r, dt, mut="trunc")
    for name in ("y", "dx"):
        share = assert_mutant(emu[name], model[name], ALL, name, dt)
        print(f"truncating store {dt} rms {name}: {100 * share:.0f} % outside")
    assert_mutant(emu["dgamma"], model["dgamma"], NONE, "dgamma", required=False)


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("mode", ["affine", "adaln", "both"])
def test_c2_from_dy_outside(mode, dt):
    d = B.make_ln(768, 50, 7, dt)
    kw = B.ln_args(d, mode, True)
    model = B.ln_bwd(d["x"], d["dy"], **kw)
    emu = emu_ln(d, mut="c2_from_dy", **kw)
    share = assert_mutant(emu["dx"], model["dx"], ALL, "dx")
    for name in model:
        if name != "dx":
            assert_mutant(emu[name], model[name], NONE, name, required=False)
    print(f"c2 from dy {mode} {dt}: {100 * share:.0f} % of dx outside")


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("case", [(37, 2, 32), (41, 12, 64)], ids=_ids([(37, 2, 32), (41, 12, 64)]))
def test_dgamma_without_sqrt_d_outside(case, dt):
    r = B.make_rms(*case, dt)
    model = B.rms_fwd_bwd(r["x"], r["dy"], r["gamma"], dt)
    emu = emu_rms(r, dt, mut="no_sqrt_d")
    assert_mutant(emu["dgamma"], model["dgamma"], ALL, "dgamma")
    for name in ("y", "dx"):
        assert_mutant(emu[name], model[name], NONE, name, dt, required=False)


# ---- the gap, shown ------------------------------------------------------------------------------------------------------------------------------

def _positions(shape):
    r, c = shape[0], int(np.prod(shape[1:]))
    return [(0, 0), (r // 2, c // 3), (r - 1, c - 1), (r - 1, 0), (0, c - 1)]


def _plant(emu, ref, bnd, pos):
    """the emulation (float64) with the element at pos moved by twice its own bound, away from the reference"""
    out = emu.double().reshape(ref.shape[0], -1).clone()
    ref2, bnd2 = ref.reshape(out.shape), bnd.reshape(out.shape)
    sign = 1.0 if out[pos] >= ref2[pos] else -1.0
    out[pos] += sign * 2.0 * bnd2[pos]
    return out.reshape(ref.shape)


def _gap(name, emu, model, yard, dt, must_pass_old):
    ref, bnd = model[0], model[-1]
    for pos in _positions(ref.shape):
        moved = _plant(emu, ref, bnd, pos)
        bad = outside(moved, model, dt).reshape(ref.shape[0], -1)
        assert int(bad.sum()) == 1 and bool(bad[pos]), f"{name} {pos}: the element-wise check flags {int(bad.sum())} elements"
        try:
            _check("gap", name, moved, ref, yard, [])
            seen = False
        except AssertionError:
            seen = True
        print(f"{name} {dt} at {pos}: moved by 2 x bound = {2 * float(bnd.reshape(ref.shape[0], -1)[pos]):.2e}; the relative-L2 bar {'SEES' if seen else 'does not see'} it")
        if must_pass_old:
            assert not seen, f"{name} {pos}: the planted error fails the old bar too"


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_a_single_element_off_by_twice_its_bound_is_caught_here_and_not_by_the_l2_bar(dt):
    """Plain inputs, whole blocks of 32 rows (the L2 bar's unit; in a last block of ONE row the bar of an fp32 output is itself nearly
    element-wise and does see the planted error).  Asserted for the fp32 dx, the 16-bit dh and the RMSNorm dx; printed for the rest."""
    C, rows, rpg = 1024, 64, 33
    d = B.make_ln(C, rows, rpg, dt, plain=True)
    kw = B.ln_args(d, "both", True)
    model = B.ln_bwd(d["x"], d["dy"], **kw)
    emu = emu_ln(d, **kw)
    shift = torch.zeros_like(d["scale"])
    yard = R.ln_mod(d["x"], d["dy"].float(), dtype=F32, lp=dt, shift=shift, **kw)
    for name in model:
        _gap(f"ln {name}", emu[name], model[name], yard[name].reshape(model[name][0].shape), dt, name == "dx")
    g = B.make_gate(C, rows, rpg, dt, plain=True)
    model = B.gate_fwd_bwd(g["x"], g["h"], g["dout"], g["gate"], rpg, dt)
    emu = emu_gate(g, True, dt)
    yard = R.gate(g["x"], g["h"].float(), g["dout"], g["gate"], rpg, dtype=F32, lp=dt)
    for name in ("dh", "dgate"):
        _gap(f"gate {name}", emu[name], model[name], yard[name], dt, name == "dh")
    r = B.make_rms(64, 16, 64, dt, plain=True)
    model = B.rms_fwd_bwd(r["x"], r["dy"], r["gamma"], dt)
    emu = emu_rms(r, dt)
    yard = R.rms(r["x"].float(), r["dy"].float(), r["gamma"], dtype=F32, lp=dt)
    for name in ("dx", "y", "dgamma"):
        _gap(f"rms {name}", emu[name], model[name], yard[name].reshape(model[name][0].shape), dt, name == "dx")


# ---- interval width ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_share_of_wide_intervals_on_plain_inputs(dt):
    """From the reference alone.  An element whose interval holds two values is still checked (it must be one of the two)."""
    for case in B.LN_CASES:
        g = B.make_gate(*case, dt, plain=True)
        ref, _ = B.gate_fwd_bwd(g["x"], g["h"], g["dout"], g["gate"], case[2], dt)["dh"]
        share = B.ambiguous_share(ref, B.U32 * ref.abs() * B.SECOND, dt)
        print(f"gate dh {case} {dt}: {100 * share:.3f} % of the intervals hold two values")
        assert share < 0.05
    for case in B.RMS_CASES:
        r = B.make_rms(*case, dt, plain=True)
        model = B.rms_fwd_bwd(r["x"], r["dy"], r["gamma"], dt)
        for name in ("y", "dx"):
            share = B.ambiguous_share(model[name][0], model[name][1], dt)
            print(f"rms {name} {case} {dt}: {100 * share:.3f} % of the intervals hold two values")
            assert share < 0.05
