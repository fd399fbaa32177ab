"""Host reference of the sparse path's wiring, written from the definitions -- it never calls calc_window_partition or calc_serialization.

A *span* is (batch, key rows, write rows): the rows one attention sequence reads as keys, in sequence order, and the rows whose output it
writes back.  For a window of the swin partition both are the window's tokens; for a window of a serialisation the keys are `window_size`
modular positions of the sample in curve order and the writes are its valid span (sparse/attention/serialized_attn.py); for full attention
both are the sample.

window_groups / serial_codes / serial_spans / sample_spans / spans_of_rule   the spans of a plan, from coordinates
check_plan                                                                   exact: a product plan (fwd, bwd, lens) against the spans
plan_of_spans / run_plan                                                     a plan from spans; attention through a plan (for mutants)
per_group / assert_per_group / chunk_groups                                  the measure: relative L2 per group of rows against the yardstick's
MARGIN                                                                       m of the bar E_g <= m * max(Y_g, median_g Y): DESIGN.md section 5
"""
import math

import numpy as np
import torch

# the permute of the four SerializeModes (serialized_attn.py:28-29): the curve and the axis order its encoder is handed
ORDERS = {"Z_ORDER": ("z_order", (0, 1, 2)), "Z_ORDER_TRANSPOSED": ("z_order", (1, 0, 2)),
          "HILBERT": ("hilbert", (0, 1, 2)), "HILBERT_TRANSPOSED": ("hilbert", (1, 0, 2))}

# Measured on the CPU (tests/test_sparse_ref.py::test_margin_between_two_cpu_implementations, over the block cases of
# tests/test_sparse_conformance_gpu.py): the largest E_g / max(Y_g, median Y) of oracle.sparse_vae_ref.block with spans against float64 with
# the TorchOps wiring as yardstick, and the other way round: 1.238 and 1.376; m = the larger + 50 %, not below the project's 2 (DESIGN.md
# section 5).
MARGIN = 2.064


def layout_of(coords):
    """[(start, stop)] per sample of batch-sorted coords (T, 4)"""
    b = coords[:, 0].long()
    assert bool((b[1:] >= b[:-1]).all())
    counts = torch.bincount(b, minlength=int(b.max()) + 1 if b.numel() else 0).tolist()
    ends = np.cumsum(counts).tolist()
    return list(zip([0] + ends[:-1], ends))


def sample_spans(layout, kv_layout=None):
    """full attention: one span a sample (kv_layout: the context's rows, for the cross forms)"""
    kv_layout = layout if kv_layout is None else kv_layout
    return [(b, torch.arange(k0, k1), torch.arange(s0, s1)) for b, ((s0, s1), (k0, k1)) in enumerate(zip(layout, kv_layout))]


def window_groups(coords, window, shift):
    """The sets of rows that share (batch, floor((xyz + shift) / window)), in ascending (batch, wx, wy, wz); rows ascending inside a set."""
    shift = (shift,) * 3 if isinstance(shift, int) else tuple(shift)
    window = (window,) * 3 if isinstance(window, int) else tuple(window)
    groups = {}
    for t, (b, x, y, z) in enumerate(coords.tolist()):
        key = (b, (x + shift[0]) // window[0], (y + shift[1]) // window[1], (z + shift[2]) // window[2])
        groups.setdefault(key, []).append(t)
    return [(key[0], torch.tensor(rows), torch.tensor(rows)) for key, rows in sorted(groups.items())]


def serial_codes(oracle_lib, coords, order, shift_window=(0, 0, 0)):
    """The curve code of every row: the C oracle's encoder on xyz + shift_window in the axis order of `order` (a name of ORDERS)."""
    mode, permute = ORDERS[order]
    c = coords[:, 1:].long() + torch.tensor(shift_window).reshape(1, 3)
    return torch.from_numpy(oracle_lib.vox2seq_encode(c[:, list(permute)].numpy(), mode).astype(np.int64))


def serial_spans(codes, layout, window, shift_sequence=0):
    """Per sample and per window the `window` key rows and the rows that window writes back, restated from the rule documented in
    sparse/attention/serialized_attn.py: a sample of n rows in code order is cut into nw = ceil(n / window) windows; window i is centred on
    (i + 0.5) n / nw + shift_sequence, its keys are the `window` modular positions from floor(centre - window / 2), and it writes the
    positions split[i] .. split[i + 1] (modulo n) with split[i] = floor(i n / nw + shift_sequence).  A sample that fits one window is a
    single span over all its rows."""
    spans = []
    for b, (s0, s1) in enumerate(layout):
        n = s1 - s0
        order = torch.sort(codes[s0:s1], stable=True).indices + s0
        nw = -(-n // window)
        if nw <= 1:
            spans.append((b, order, order))
            continue
        valid = n / nw
        for i in range(nw):
            start = math.floor((i + 0.5) * valid + shift_sequence - 0.5 * window)
            keys = order[torch.arange(start, start + window) % n]
            lo, hi = math.floor(i * valid + shift_sequence), math.floor((i + 1) * valid + shift_sequence)
            spans.append((b, keys, order[torch.arange(lo, hi) % n]))
    return spans


def spans_of_rule(oracle_lib, coords, rule):
    """The spans of one block's plan (oracle.sparse_vae_ref.block_attn_rule's dict, or one written by hand)."""
    if rule["kind"] == "full":
        return sample_spans(layout_of(coords))
    if rule["kind"] == "windowed":
        return window_groups(coords, rule["window"], rule.get("shift") or 0)
    codes = serial_codes(oracle_lib, coords, rule.get("order") or "Z_ORDER", rule.get("shift_window") or (0, 0, 0))
    return serial_spans(codes, layout_of(coords), rule["window"], rule.get("shift_sequence") or 0)


def check_plan(fwd, bwd, lens, spans, T, ordered, batch_idx=None):
    """Exact.  The sequences of `lens`, read from `fwd`, are the spans' key sets, one sequence per span in the same order (and on the same
    batch element, when batch_idx is given); inside a sequence the order is the span's (ordered: a serialisation) or free (a window
    partition, whose reference leaves it unspecified).  Every token has exactly one bwd entry, fwd[bwd[t]] == t, and bwd[t] lies in the
    sequence whose write set holds t.  fwd / bwd None (full attention): the sequences are the samples in place."""
    lens = [int(n) for n in lens]
    assert len(lens) == len(spans), f"{len(lens)} sequences for {len(spans)} spans"
    if batch_idx is not None:
        assert [int(b) for b in batch_idx] == [s[0] for s in spans], "batch indices of the sequences"
    if fwd is None:
        assert bwd is None and sum(lens) == T
        fwd = bwd = torch.arange(T)
    fwd, bwd = fwd.cpu().long(), bwd.cpu().long()
    assert fwd.dim() == 1 and fwd.numel() == sum(lens), f"fwd holds {fwd.numel()} rows, the sequences {sum(lens)}"
    assert bwd.shape == (T,), f"bwd holds {tuple(bwd.shape)} entries for {T} tokens"
    assert fwd.numel() == 0 or (0 <= int(fwd.min()) and int(fwd.max()) < T), "fwd out of range"
    assert T == 0 or (0 <= int(bwd.min()) and int(bwd.max()) < fwd.numel()), "bwd out of range"
    writer = torch.full((T,), -1, dtype=torch.long)
    seq_of = torch.empty((fwd.numel(),), dtype=torch.long)
    off = 0
    for i, (n, (_, keys, writes)) in enumerate(zip(lens, spans)):
        seq = fwd[off:off + n]
        assert n == keys.numel(), f"sequence {i}: {n} rows, the span has {keys.numel()} keys"
        if ordered:
            assert torch.equal(seq, keys), f"sequence {i}: rows or their order differ from the span's keys"
        else:
            assert torch.equal(seq.sort().values, keys.sort().values), f"sequence {i}: not the span's key set"
        assert bool((writer[writes] == -1).all()), f"span {i} writes a row another span writes"
        writer[writes] = i
        seq_of[off:off + n] = i
        off += n
    assert bool((writer >= 0).all()), "a token no span writes"
    assert torch.equal(fwd[bwd], torch.arange(T)), "fwd[bwd[t]] != t"
    bad = torch.nonzero(seq_of[bwd] != writer).squeeze(1)
    assert bad.numel() == 0, f"bwd takes {bad.numel()} tokens (first {int(bad[0]) if bad.numel() else -1}) from a sequence that does not write them"


def plan_of_spans(spans, T):
    """(fwd, bwd, lens): the plan that realises the spans, sequences in span order"""
    fwd = torch.cat([k for _, k, _ in spans])
    bwd = torch.full((T,), -1, dtype=torch.long)
    off = 0
    for _, keys, writes in spans:
        pos = {int(r): off + j for j, r in enumerate(keys.tolist())}
        bwd[writes] = torch.tensor([pos[int(r)] for r in writes.tolist()])
        off += keys.numel()
    return fwd, bwd, [int(k.numel()) for _, k, _ in spans]


def run_plan(q, k, v, fwd, bwd, lens, precision):
    """What a plan computes: gather into sequence order, attention per sequence, out[bwd] (the product's three steps, on the host)."""
    from oracle import sparse_vae_ref as ref
    qs, ks, vs = q[fwd], k[fwd], v[fwd]
    cu = np.concatenate([[0], np.cumsum(lens)]).tolist()
    seqs = [(0, torch.arange(a, b), torch.arange(a, b)) for a, b in zip(cu[:-1], cu[1:])]
    return ref.attention_spans(qs, ks, vs, seqs, precision)[bwd]


# ---- the measure ------------------------------------------------------------------------------------------------------------------------
def chunk_groups(layout, chunk=16):
    """the samples, and fixed chunks of `chunk` consecutive rows: the groups of a multi-block result, where windows of different blocks mix"""
    T = layout[-1][1] if layout else 0
    return [torch.arange(s0, s1) for s0, s1 in layout] + [torch.arange(r, min(r + chunk, T)) for r in range(0, T, chunk)]


def write_groups(spans):
    return [w for _, _, w in spans]


def _rel_rows(x, ref, rows):
    x, ref = x[rows].double().reshape(-1), ref[rows].double().reshape(-1)
    num, den = float((x - ref).norm()), float(ref.norm())
    return 0.0 if num == 0.0 else (num / den if den > 0 else float("inf"))


def per_group(got, r64, yard, groups, m=None):
    """For every group g of rows: E_g = relative L2 of `got` against `r64` over those rows, Y_g the same for the yardstick; the bar is
    E_g <= m * max(Y_g, median_g Y) (the median floor keeps a one-token window whose yardstick happens to be tiny from failing a correct
    kernel).  The groups must cover every row.  -> dict(ratio: the largest E_g / max(Y_g, median Y), bad: the groups over the bar as
    (index, E_g, Y_g), E / Y: the whole-tensor figures, median)."""
    m = MARGIN if m is None else m
    got, r64, yard = (t.detach().cpu() for t in (got, r64, yard))
    assert got.shape == r64.shape == yard.shape, (got.shape, r64.shape, yard.shape)
    covered = torch.zeros((got.shape[0],), dtype=torch.bool)
    for rows in groups:
        covered[rows] = True
    assert bool(covered.all()), "a row outside every group: the cap on skipped groups is zero"
    E = [_rel_rows(got, r64, rows) for rows in groups]
    Y = [_rel_rows(yard, r64, rows) for rows in groups]
    med = float(np.median(Y))
    ratio, bad = 0.0, []
    for i, (e, y) in enumerate(zip(E, Y)):
        unit = max(y, med)
        r = 0.0 if e == 0.0 else (e / unit if unit > 0 else float("inf"))
        ratio = max(ratio, r)
        if not r <= m:                                                   # (also a NaN)
            bad.append((i, e, y))
    everything = torch.arange(got.shape[0])
    return dict(ratio=ratio, bad=bad, E=_rel_rows(got, r64, everything), Y=_rel_rows(yard, r64, everything), median=med, m=m)


def assert_per_group(what, got, r64, yard, groups, m=None):
    assert bool(torch.isfinite(got).all()), f"{what}: not finite"
    r = per_group(got, r64, yard, groups, m)
    i, e, y = r["bad"][0] if r["bad"] else (-1, 0.0, 0.0)
    assert not r["bad"], (f"{what}: {len(r['bad'])} of {len(groups)} groups over {r['m']} x max(Y_g, median {r['median']:.2e}); first: group {i} "
                          f"({groups[i].numel() if i >= 0 else 0} rows) E {e:.3e} Y {y:.3e}; whole tensor {r['E']:.2e} / {r['Y']:.2e}")
    return r["ratio"]


# ---- the cases shared by tests/test_sparse_ref.py (the CPU margin) and tests/test_sparse_conformance_gpu.py ------------------------------
SIZES = (150, 90, 1, 64, 65, 128)     # one voxel; n == window, n == window + 1 and an exact multiple of the serialised windows 64 and 32
WIDTHS = {128: 2, 64: 2}              # channels -> heads: head_dim 64 and 32
BLOCK_MODES = ("swin", "shift_window", "shift_sequence", "shift_order", "full")


def voxels(res, counts=SIZES, seed=5):
    """distinct random voxels per sample on a res^3 grid, batch-sorted (T, 4) int32"""
    g = torch.Generator().manual_seed(seed)
    out = []
    for b, n in enumerate(counts):
        c = torch.unique(torch.randint(0, res, (n * 3 + 8, 3), generator=g), dim=0)
        c = c[torch.randperm(c.shape[0], generator=g)[:n]]
        assert c.shape[0] == n
        out.append(torch.cat([torch.full((n, 1), b), c], dim=1))
    return torch.cat(out).int()


def grid_of(mode_or_rule):
    """16^3, or 32^3 where a window shift of 16 is used (on 16^3 it would move every voxel into the same octant: no change of order)"""
    if isinstance(mode_or_rule, dict):
        return 32 if tuple(mode_or_rule.get("shift_window") or (0, 0, 0)) != (0, 0, 0) and mode_or_rule["kind"] == "serialized" else 16
    return 32 if mode_or_rule == "shift_window" else 16


def block_cfg(mode, C):
    """the backbone configuration whose block i the block cases run: window 8 (swin), serialised windows of 64 (C = 128) or 32 (C = 64)"""
    return dict(attn_mode=mode, window_size=8 if mode == "swin" else (64 if C == 128 else 32), model_channels=C, num_heads=WIDTHS[C])


def block_state(C, seed=21, ctx_channels=None):
    """(state dict of one block incl. both RMSNorm gains and the cross projections, x (T, C), loss weights w (T, C)) for T = sum(SIZES)"""
    g = torch.Generator().manual_seed(seed + C)
    T, H = sum(SIZES), WIDTHS[C]
    x, w = torch.randn((T, C), generator=g), torch.randn((T, C), generator=g)
    shapes = {"attn.to_qkv.weight": (3 * C, C), "attn.to_qkv.bias": (3 * C,), "attn.to_out.weight": (C, C), "attn.to_out.bias": (C,),
              "mlp.mlp.0.weight": (4 * C, C), "mlp.mlp.0.bias": (4 * C,), "mlp.mlp.2.weight": (C, 4 * C), "mlp.mlp.2.bias": (C,),
              "attn.to_q.weight": (C, C), "attn.to_q.bias": (C,), "attn.to_kv.weight": (2 * C, ctx_channels or C), "attn.to_kv.bias": (2 * C,)}
    sd = {k: torch.randn(s, generator=g) * (s[1] ** -0.5 if len(s) == 2 else 0.1) for k, s in shapes.items()}
    for k in ("attn.q_rms_norm.gamma", "attn.k_rms_norm.gamma"):
        sd[k] = 1 + 0.1 * torch.randn((H, C // H), generator=g)
    return sd, x, w


def module_kwargs(rule):
    """the constructor keywords of SparseMultiHeadAttention / SparseTransformerBlock for a rule"""
    from gvfdiffusion_amd.sparse.attention import SerializeMode
    if rule["kind"] == "full":
        return dict(attn_mode="full")
    if rule["kind"] == "windowed":
        return dict(attn_mode="windowed", window_size=rule["window"], shift_window=rule.get("shift") or 0)
    return dict(attn_mode="serialized", window_size=rule["window"], shift_sequence=rule.get("shift_sequence") or 0,
                shift_window=tuple(rule.get("shift_window") or (0, 0, 0)), serialize_mode=SerializeMode[rule.get("order") or "Z_ORDER"])


def block_keys(sd, rms):
    return [k for k in sd if not k.startswith(("attn.to_q.", "attn.to_kv.")) and (rms or "rms_norm" not in k)]


def oracle_block(x, w, sd, spans, H, precision, old, rms, dtype):
    """oracle.sparse_vae_ref.block over the spans with autograd on leaves of `dtype` -> dict y, x (the input gradient of sum(y * w)), and
    every parameter gradient"""
    from oracle import sparse_vae_ref as ref
    keys = block_keys(sd, rms)
    leaves = {"b." + k: sd[k].to(dtype).requires_grad_() for k in keys}
    xi = x.to(dtype).requires_grad_()
    y = ref.block(xi, spans, leaves, "b", H, precision, old, rms)
    out = dict(zip(keys + ["x"], torch.autograd.grad((y * w.to(dtype)).sum(), [leaves["b." + k] for k in keys] + [xi])))
    out["y"] = y.detach()
    return out


def torch_block(x, w, sd, coords, rule, spans, H, old, rms, dtype, lp):
    """The product's own training wiring (block_rows) through tests/sparse_train_ref.py::TorchOps on the CPU, over the plan the spans
    define (registered on the tensor: nothing of calc_window_partition / calc_serialization runs) -> the dict of oracle_block."""
    import sparse_train_ref as R
    from gvfdiffusion_amd import sparse as sp
    from gvfdiffusion_amd.model.sparse_voxel_diffusion import SparseTransformerBlock
    C = x.shape[1]
    b = SparseTransformerBlock(C, num_heads=H, modulated=False, use_old_attn_impl=old, qk_rms_norm=rms, **module_kwargs(rule))
    b.load_state_dict({k: sd[k] for k in block_keys(sd, rms)})
    b = b.to(dtype)
    st = sp.SparseTensor(x.to(dtype), coords)
    a = b.attn
    fwd, bwd, lens = (None, None, [int(k.numel()) for _, k, _ in spans]) if rule["kind"] == "full" else plan_of_spans(spans, x.shape[0])
    cu = torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int32)
    st.register_spatial_cache(f"rows_{a.attn_mode}_{a.window_size}_{a.shift_sequence}_{a.shift_window}_{a.serialize_mode}",
                              (fwd, bwd, cu, int(max(lens))))
    xi = x.to(dtype).requires_grad_()
    y = b.forward_rows_train(xi, st, lp, ops=R.TorchOps())
    names, params = zip(*b.named_parameters())
    out = dict(zip(names + ("x",), torch.autograd.grad((y * w.to(dtype)).sum(), list(params) + [xi])))
    out["y"] = y.detach()
    return out
