"""The host reference of the sparse path's wiring (tests/sparse_ref.py, oracle/sparse_vae_ref.py::attention_spans) on the CPU: pinned to the
reference project's own plans (tests/golden/sparse_index_golden.npz), shown to reject seven wiring mutants (with the whole-tensor relative L2 each one produces printed beside the verdict),
and the measurement of the per-group margin m between two independent correct implementations at operand precision."""
import os

import numpy as np
import pytest
import torch

import sparse_ref as S

G = np.load(os.path.join(os.path.dirname(__file__), "golden", "sparse_index_golden.npz"))
OLD_BAR = 6e-3                       # the whole-sequence relative L2 tests/test_sparse.py holds the attention functions to (bf16)
SER_GOLDEN = ((32, 0, (0, 0, 0)), (48, 7, (3, 0, 5)))


def _gold(key):
    return torch.from_numpy(G[key + "_fwd"]), torch.from_numpy(G[key + "_bwd"]), G[key + "_lens"].tolist(), G[key + "_bidx"].tolist()


def test_check_plan_accepts_the_reference_projects_plans(oracle_lib):
    coords = torch.from_numpy(G["coords"])
    T = coords.shape[0]
    seen = set()
    for key, ws, sh in (("win_8_0", 8, 0), ("win_8_4", 8, 4), ("win_5_1_2_3", 5, (1, 2, 3))):
        fwd, bwd, lens, bidx = _gold(key)
        S.check_plan(fwd, bwd, lens, S.window_groups(coords, ws, sh), T, False, bidx)
        seen.add(key)
    for order in S.ORDERS:
        for ws, ss, sw in SER_GOLDEN:
            key = f"ser_{order}_{ws}_{ss}"
            fwd, bwd, lens, bidx = _gold(key)
            spans = S.serial_spans(S.serial_codes(oracle_lib, coords, order, sw), S.layout_of(coords), ws, ss)
            S.check_plan(fwd, bwd, lens, spans, T, True, bidx)
            seen.add(key)
    assert seen == {k[:-4] for k in G.files if k.endswith("_fwd")}            # every plan of the fixture


def test_spans_at_the_edges(oracle_lib):
    """one voxel, n == window, n == window + 1, an exact multiple under a shifted sequence: what the spans are, by hand"""
    coords = S.voxels(16, (1, 64, 65, 128), 3)
    lay = S.layout_of(coords)
    codes = S.serial_codes(oracle_lib, coords, "HILBERT")
    spans = S.serial_spans(codes, lay, 64, 32)
    assert [(b, k.numel(), w.numel()) for b, k, w in spans] == [(0, 1, 1), (1, 64, 64), (2, 64, 32), (2, 64, 33), (3, 64, 64), (3, 64, 64)]
    order = torch.sort(codes[lay[3][0]:lay[3][1]], stable=True).indices + lay[3][0]
    assert torch.equal(spans[4][1], order[32:96]) and torch.equal(spans[5][1], torch.cat([order[96:], order[:32]]))     # the wrap
    assert torch.equal(spans[4][1], spans[4][2]) and torch.equal(spans[5][1], spans[5][2])
    fwd, bwd, lens = S.plan_of_spans(spans, coords.shape[0])
    S.check_plan(fwd, bwd, lens, spans, coords.shape[0], True)
    assert sum(w.numel() for _, _, w in spans) == coords.shape[0]
    # n == window + 1 without a shift: two windows of 64 keys over 65 rows, writing 32 and 33
    s2 = S.serial_spans(codes, lay, 64, 0)[2:4]
    o2 = torch.sort(codes[lay[2][0]:lay[2][1]], stable=True).indices + lay[2][0]
    assert torch.equal(s2[0][2], o2[:32]) and torch.equal(s2[1][2], o2[32:])
    assert torch.equal(s2[0][1], o2[torch.arange(-16, 48) % 65]) and torch.equal(s2[1][1], o2[torch.arange(16, 80) % 65])


# ---- mutants ------------------------------------------------------------------------------------------------------------------------------
def _qkv(T, H, d, seed):
    g = torch.Generator().manual_seed(seed)
    return tuple(torch.randn((T, H, d), generator=g).to(torch.bfloat16).float() for _ in range(3))


def _verdicts(name, got, r64, yard, groups, plan=None, spans=None, ordered=True, T=None, old_bar=None):
    """-> (per-group verdict, check_plan verdict or None, whole-tensor relative L2, whether the old whole-tensor bar passes it): True =
    rejected.  old_bar None: the attention functions' 6e-3; a number: that multiple of the whole-tensor yardstick (the blocks' 2)."""
    r = S.per_group(got, r64, yard, groups)
    plan_rejected = None
    if plan is not None:
        try:
            S.check_plan(*plan, spans, T, ordered)
            plan_rejected = False
        except AssertionError:
            plan_rejected = True
    bar = OLD_BAR if old_bar is None else old_bar * r["Y"]
    old = "passes" if r["E"] < bar else "fails"
    print(f"mutant | {name:58s} | per-group {'REJECTS' if r['bad'] else 'accepts'} ({len(r['bad'])} of {len(groups)} groups, worst ratio "
          f"{r['ratio']:.1f} against m = {r['m']}) | check_plan {'-' if plan_rejected is None else ('REJECTS' if plan_rejected else 'accepts')}"
          f" | whole-tensor rel L2 {r['E']:.2e} (yardstick {r['Y']:.2e}): {old} the old bar {bar:.2g}")
    return bool(r["bad"]), plan_rejected, r["E"], r["E"] < bar


def test_wiring_mutants_are_rejected(oracle_lib):
    """Each mutant is applied to a correct result or plan on the batch of the GPU cases (150, 90, 1, 64, 65, 128 voxels, 2 heads of 64, bf16
    operands).  The per-group measure, or check_plan where the mutant is a plan, must reject every one; the whole-tensor figure each one
    produces is printed next to the 6e-3 the attention functions were held to (run with -s for the table; DESIGN.md section 5 records it)."""
    from oracle import sparse_vae_ref as ref
    coords = S.voxels(16)
    T, H, d = coords.shape[0], 2, 64
    lay = S.layout_of(coords)
    q, k, v = _qkv(T, H, d, 1)
    q64, k64, v64 = q.double(), k.double(), v.double()
    win = S.window_groups(coords, 8, 4)
    ser = S.serial_spans(S.serial_codes(oracle_lib, coords, "Z_ORDER"), lay, 64, 0)
    win64, ser64 = ref.attention_spans(q64, k64, v64, win, "fp32"), ref.attention_spans(q64, k64, v64, ser, "fp32")
    win16, ser16 = ref.attention_spans(q, k, v, win, "bf16"), ref.attention_spans(q, k, v, ser, "bf16")
    gw, gs = S.write_groups(win), S.write_groups(ser)
    # the correct results are accepted, and a correct plan through the plan executor is the same thing
    assert not S.per_group(win16, win64, win16, gw)["bad"] and not S.per_group(ser16, ser64, ser16, gs)["bad"]
    plan = S.plan_of_spans(ser, T)
    S.check_plan(*plan, ser, T, True)
    assert torch.equal(S.run_plan(q, k, v, *plan, "bf16"), ser16)
    seen = {}

    # 1. one key dropped from one window (the largest: the smallest change)
    i = max(range(len(win)), key=lambda j: win[j][1].numel())
    m1 = list(win)
    m1[i] = (win[i][0], win[i][1][1:], win[i][2])
    seen["one key dropped from one window"] = _verdicts(f"one key dropped from one window ({win[i][1].numel()} keys)",
                                                        ref.attention_spans(q, k, v, m1, "bf16"), win64, win16, gw)
    # 2. two rows of different windows swapped in bwd
    fwd, bwd, lens = S.plan_of_spans(win, T)
    b2 = bwd.clone()
    t0, t1 = int(win[0][2][0]), int(win[-1][2][0])
    b2[t0], b2[t1] = bwd[t1], bwd[t0]
    seen["two rows of different windows swapped in bwd"] = _verdicts(
        "two rows of different windows swapped in bwd", S.run_plan(q, k, v, fwd, b2, lens, "bf16"), win64, win16, gw,
        plan=(fwd, b2, lens), spans=win, ordered=False, T=T)
    # 3. a serialised window writing its whole span (it lands on its neighbours' valid rows)
    j = next(j for j, (_, kk, ww) in enumerate(ser) if ww.numel() < kk.numel())
    m3 = list(ser) + [(ser[j][0], ser[j][1], ser[j][1])]
    seen["a serialised window writing its whole span"] = _verdicts(
        f"a serialised window writing its whole span ({ser[j][1].numel()} rows for {ser[j][2].numel()})",
        ref.attention_spans(q, k, v, m3, "bf16"), ser64, ser16, gs)
    # 4. the shift on the wrong block parity: block 0 of a swin backbone run over block 1's windows
    sd, x, w = S.block_state(128)
    even = S.window_groups(coords, 8, 0)
    b64 = S.oracle_block(x, w, sd, even, H, "fp32", True, False, torch.float64)
    b16 = S.oracle_block(x, w, sd, even, H, "bf16", True, False, torch.float32)
    bad = S.oracle_block(x, w, sd, win, H, "bf16", True, False, torch.float32)
    for what in ("y", "x"):
        assert not S.per_group(b16[what], b64[what], b16[what], S.write_groups(even))["bad"]
        seen[f"shift on the wrong parity ({what})"] = _verdicts(f"the shift on the wrong block parity, block {'output' if what == 'y' else 'input gradient'}",
                                                                bad[what], b64[what], b16[what], S.write_groups(even), old_bar=2)
    # 1b / 3b / 5b. the local mutants inside a block, where the residual stream carries most of the norm: the blocks' old bar is 2 x the
    # whole-tensor yardstick
    w64 = S.oracle_block(x, w, sd, win, H, "fp32", True, False, torch.float64)
    s64 = S.oracle_block(x, w, sd, ser, H, "fp32", True, False, torch.float64)
    s16 = S.oracle_block(x, w, sd, ser, H, "bf16", True, False, torch.float32)
    e5 = next(j for j in range(len(win) - 1) if win[j][0] != win[j + 1][0])
    both5 = torch.cat([win[e5][1], win[e5 + 1][1]])
    for tag, spans_m, r_, y_, gr in (("one key dropped from one window", m1, w64, bad, gw), ("a serialised window writing its whole span", m3, s64, s16, gs),
                                     ("edge windows of two samples merged", win[:e5] + [(win[e5][0], both5, both5)] + win[e5 + 2:], w64, bad, gw)):
        mb = S.oracle_block(x, w, sd, spans_m, H, "bf16", True, False, torch.float32)
        for what in ("y", "x"):
            seen[f"{tag}, block ({what})"] = _verdicts(f"{tag}, block {'output' if what == 'y' else 'input gradient'}",
                                                       mb[what], r_[what], y_[what], gr, old_bar=2)
    # 5. the last window of sample b merged with the first of sample b + 1
    e = next(j for j in range(len(win) - 1) if win[j][0] != win[j + 1][0])
    both = torch.cat([win[e][1], win[e + 1][1]])
    m5 = win[:e] + [(win[e][0], both, both)] + win[e + 2:]
    seen["edge windows of two samples merged"] = _verdicts(
        f"last window of sample {win[e][0]} merged with the first of {win[e + 1][0]} ({win[e][1].numel()} + {win[e + 1][1].numel()} rows)",
        ref.attention_spans(q, k, v, m5, "bf16"), win64, win16, gw)
    f5, bw5, l5 = S.plan_of_spans(m5, T)
    with pytest.raises(AssertionError):
        S.check_plan(f5, bw5, l5, win, T, False)
    # 6. old and new qkv channel layout exchanged for one head
    g = torch.Generator().manual_seed(6)
    rows = torch.randn((T, 3 * H * d), generator=g).to(torch.bfloat16).float()
    new = ref._heads(rows, 3, H, False)
    old = ref._heads(rows, 3, H, True)
    mixed = [torch.stack([new[p][:, 0], old[p][:, 1]], dim=1) for p in range(3)]          # head 1 read in the other layout
    l64 = ref.attention_spans(*(t.double() for t in new), win, "fp32")
    l16 = ref.attention_spans(*new, win, "bf16")
    seen["layouts exchanged for one head"] = _verdicts("old and new qkv channel layout exchanged for one head",
                                                       ref.attention_spans(*mixed, win, "bf16"), l64, l16, gw)
    # 7. a plan from other coordinates with the same layout sizes
    other = S.voxels(16, seed=77)
    assert S.layout_of(other) == lay and not torch.equal(other, coords)
    ow = S.window_groups(other, 8, 4)
    po = S.plan_of_spans(ow, T)
    # (another window count: the executor runs the foreign plan as it stands, check_plan compares it with this tensor's spans)
    seen["a plan from other coordinates"] = _verdicts("a plan from other coordinates with the same layout sizes",
                                                      S.run_plan(q, k, v, *po, "bf16"), win64, win16, gw, plan=po, spans=win, ordered=False, T=T)
    so = S.serial_spans(S.serial_codes(oracle_lib, other, "Z_ORDER"), lay, 64, 0)
    ps = S.plan_of_spans(so, T)                                                        # same lens, same count: only the rows differ
    assert ps[2] == plan[2]
    seen["a serialisation from other coordinates"] = _verdicts("a serialisation from other coordinates (equal lens)",
                                                               S.run_plan(q, k, v, *ps, "bf16"), ser64, ser16, gs, plan=ps, spans=ser, T=T)
    for name, (group_rejects, plan_rejects, _, _) in seen.items():
        assert group_rejects, f"{name}: the per-group measure accepts it"
        assert plan_rejects in (None, True), f"{name}: check_plan accepts it"
    # the record of what the old whole-tensor measure passes at these sizes (printed, not asserted: it is a property of the old bar)
    print("mutant | passed by the old whole-tensor bar:", [name for name, v in seen.items() if v[3]])


# ---- the margin ---------------------------------------------------------------------------------------------------------------------------
def _block_cases():
    from oracle import sparse_vae_ref as ref
    for mode in S.BLOCK_MODES:
        for C in S.WIDTHS:
            for i in (0, 1):
                yield mode, C, i, ref.block_attn_rule(S.block_cfg(mode, C), i)


def test_margin_between_two_cpu_implementations(oracle_lib):
    """m is measured here, on the CPU, never against the HIP path: over every block case of tests/test_sparse_conformance_gpu.py (five
    backbone modes x both parities x both widths x bf16 / fp16; the block output and the input gradient), the largest
    E_g / max(Y_g, median Y) of oracle.sparse_vae_ref.block over the spans against its float64 run with the TorchOps wiring of the product's
    block_rows as the yardstick, and the other way round.  MARGIN must be that figure + 50 %, and not below the project's 2."""
    worst = {"oracle measured in TorchOps units": 0.0, "TorchOps measured in oracle units": 0.0}
    for mode, C, i, rule in _block_cases():
        H = S.WIDTHS[C]
        coords = S.voxels(S.grid_of(mode))
        spans = S.spans_of_rule(oracle_lib, coords, rule)
        groups = S.write_groups(spans)
        sd, x, w = S.block_state(C)
        old = C == 128
        r64 = S.oracle_block(x, w, sd, spans, H, "fp32", old, False, torch.float64)
        for lp, name in ((torch.bfloat16, "bf16"), (torch.float16, "fp16")):
            a = S.oracle_block(x, w, sd, spans, H, name, old, False, torch.float32)
            b = S.torch_block(x, w, sd, coords, rule, spans, H, old, False, torch.float32, lp)
            for what in ("y", "x"):
                ra = S.per_group(a[what], r64[what], b[what], groups)["ratio"]
                rb = S.per_group(b[what], r64[what], a[what], groups)["ratio"]
                worst["oracle measured in TorchOps units"] = max(worst["oracle measured in TorchOps units"], ra)
                worst["TorchOps measured in oracle units"] = max(worst["TorchOps measured in oracle units"], rb)
                print(f"margin | {mode:14s} block {i} C {C:3d} {name} {what}: {len(groups):3d} groups, oracle/TorchOps {ra:.2f}, TorchOps/oracle {rb:.2f}")
    top = max(worst.values())
    print(f"margin | largest per-group ratios: {worst}; m = max(2, 1.5 x {top:.3f}) = {max(2.0, 1.5 * top):.3f}; MARGIN = {S.MARGIN}")
    # (2 % of play: the summation order of the CPU GEMMs depends on the thread count, which moves the figure in its third digit)
    assert S.MARGIN >= 2.0 and S.MARGIN * 1.02 >= 1.5 * top, f"MARGIN {S.MARGIN} is below the measured {top:.3f} + 50 %"
    assert S.MARGIN <= max(2.0, 1.5 * top) * 1.02, f"MARGIN {S.MARGIN} is wider than the measured {top:.3f} + 50 % (and than 2)"
