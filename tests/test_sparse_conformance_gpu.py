"""The sparse path's wiring on the MI355X against the host reference written from the definitions (tests/sparse_ref.py) and the float64
oracle over its spans (oracle/sparse_vae_ref.py::attention_spans, multi_head_attention, block, torso_spans): the plans exactly, every
forward output and input gradient per window -- E_g <= m * max(Y_g, median Y) with the yardstick the same oracle at the operand type's
rounding placement and m = sparse_ref.MARGIN, measured on the CPU (tests/test_sparse_ref.py) -- and every parameter gradient on the whole
tensor at 2 x the yardstick.  The batch: samples of 150, 90, 1, 64, 65 and 128 voxels (one voxel; n == window, n == window + 1 and an exact
multiple of the serialised windows 64 and 32) on a 16^3 grid, 32^3 where a window shift of 16 is used; 128 channels in 2 heads of 64 and 64
channels in 2 heads of 32.  Each test prints the largest per-group ratio it saw (DESIGN.md section 5 records them)."""
import pytest
import torch

import sparse_ref as S
import sparse_train_ref as R

pytestmark = pytest.mark.gpu
DTYPES = [(torch.bfloat16, "bf16"), (torch.float16, "fp16")]
DT_IDS = ["bf16", "fp16"]
WIN_CFG = [dict(kind="windowed", window=8, shift=0), dict(kind="windowed", window=8, shift=4)]
SER_CFG = [dict(kind="serialized", window=w, shift_sequence=ss, shift_window=sw, order=o)
           for w in (64, 32) for ss in (0, w // 2) for sw in ((0, 0, 0), (16, 16, 16)) for o in S.ORDERS]
_CACHE = {}


def _cached(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


def _coords(rule_or_mode):
    res = S.grid_of(rule_or_mode)
    return _cached(("coords", res), lambda: S.voxels(res))


def _spans(oracle_lib, coords, rule):
    return _cached(("spans", id(coords), tuple(sorted(rule.items()))), lambda: S.spans_of_rule(oracle_lib, coords, rule))


def _sparse(feats, coords):
    from gvfdiffusion_amd.sparse import SparseTensor
    return SparseTensor(feats.cuda(), coords.cuda())


def _partition_args(rule):
    kw = S.module_kwargs(rule)
    return kw["attn_mode"], kw.get("window_size"), kw.get("shift_sequence"), kw.get("shift_window"), kw.get("serialize_mode")


# ---- A. plans -----------------------------------------------------------------------------------------------------------------------------
def _check_token_partition(st, rule, spans, T):
    from gvfdiffusion_amd.model.sparse_voxel_diffusion.sparse_transformer import token_partition
    fwd, bwd, cu, longest = token_partition(st, *_partition_args(rule))
    assert cu.dtype == torch.int32 and cu.device.type == "cuda" and int(cu[0]) == 0
    lens = (cu[1:] - cu[:-1]).tolist()
    S.check_plan(fwd, bwd, lens, spans, T, ordered=rule["kind"] != "windowed")
    assert longest == max(lens) == max(k.numel() for _, k, _ in spans)
    assert token_partition(st, *_partition_args(rule))[2] is cu                    # cached on the tensor
    return fwd, bwd, lens


def test_window_plans(cuda, oracle_lib):
    from gvfdiffusion_amd.sparse.attention import calc_window_partition
    for rule in WIN_CFG:
        coords = _coords(rule)
        T = coords.shape[0]
        spans = _spans(oracle_lib, coords, rule)
        st = _sparse(torch.zeros((T, 8)), coords)
        for shift in (rule["shift"], (rule["shift"],) * 3):
            fwd, bwd, lens, bidx = calc_window_partition(st, rule["window"], shift)
            assert isinstance(lens, list) and isinstance(bidx, list)
            S.check_plan(fwd, bwd, lens, spans, T, False, bidx)
        _check_token_partition(st, rule, spans, T)
    full = dict(kind="full")
    _check_token_partition(st, full, _spans(oracle_lib, coords, full), T)


def test_serialization_plans(cuda, oracle_lib):
    from gvfdiffusion_amd.sparse.attention import calc_serialization, SerializeMode
    for rule in SER_CFG:
        coords = _coords(rule)
        T = coords.shape[0]
        spans = _spans(oracle_lib, coords, rule)
        st = _sparse(torch.zeros((T, 8)), coords)
        fwd, bwd, lens, bidx = calc_serialization(st, rule["window"], SerializeMode[rule["order"]], rule["shift_sequence"], rule["shift_window"])
        assert isinstance(lens, list) and isinstance(bidx, list)
        S.check_plan(fwd, bwd, lens, spans, T, True, bidx)
        _check_token_partition(st, rule, spans, T)


def test_exact_multiple_under_a_shifted_sequence_is_a_permutation(cuda, oracle_lib):
    """128, 64 and 1 voxels in windows of 64 shifted by 32: every sample is a whole number of windows, the windows wrap around the sample,
    fwd is a permutation of the rows and bwd its inverse -- the case in which block_rows takes gather_rows(..., inverse)."""
    coords = S.voxels(16, (128, 64, 1), 9)
    T = coords.shape[0]
    st = _sparse(torch.zeros((T, 8)), coords)
    for order in S.ORDERS:
        rule = dict(kind="serialized", window=64, shift_sequence=32, shift_window=(0, 0, 0), order=order)
        spans = S.spans_of_rule(oracle_lib, coords, rule)
        fwd, bwd, lens = _check_token_partition(st, rule, spans, T)
        assert fwd.numel() == T and lens == [64, 64, 64, 1]
        ar = torch.arange(T, device=fwd.device)
        assert torch.equal(fwd[bwd], ar) and torch.equal(bwd[fwd], ar)


# ---- B. functions -------------------------------------------------------------------------------------------------------------------------
def _qkv(T, H, d, dt, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn((T, 3, H, d), generator=g).to(dt)


def _hold_attention(what, out, q, k, v, spans, name, worst):
    from oracle import sparse_vae_ref as ref
    r64 = ref.attention_spans(q.double(), k.double(), v.double(), spans, "fp32")
    # the functions return the operand type: the yardstick's output takes that rounding too (as the oracle's block rounds its attention output)
    yard = ref.attention_spans(q.float(), k.float(), v.float(), spans, name).to(q.dtype).float()
    assert out.shape == r64.shape and out.dtype == q.dtype
    worst.append(S.assert_per_group(what, out.float().cpu().flatten(1), r64.flatten(1), yard.flatten(1), S.write_groups(spans)))


@pytest.mark.parametrize("dt,name", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("d", [64, 32])
def test_windowed_and_serialized_functions(cuda, oracle_lib, d, dt, name):
    from gvfdiffusion_amd.sparse.attention import (sparse_windowed_scaled_dot_product_self_attention as win_attn,
                                                   sparse_serialized_scaled_dot_product_self_attention as ser_attn, SerializeMode)
    H, worst = 2, []
    for rule in WIN_CFG + SER_CFG:
        coords = _coords(rule)
        qkv = _qkv(coords.shape[0], H, d, dt, 11)
        st = _sparse(qkv, coords)
        if rule["kind"] == "windowed":
            out = win_attn(st, rule["window"], (rule["shift"],) * 3)
        else:
            out = ser_attn(st, rule["window"], SerializeMode[rule["order"]], rule["shift_sequence"], rule["shift_window"])
        _hold_attention(f"{rule} d={d} {name}", out.feats, qkv[:, 0], qkv[:, 1], qkv[:, 2], _spans(oracle_lib, coords, rule), name, worst)
    print(f"B functions windowed / serialized d={d} {name}: largest per-group ratio {max(worst):.2f} over {len(worst)} configurations (m = {S.MARGIN})")


@pytest.mark.parametrize("dt,name", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("d", [64, 32])
def test_five_call_forms_of_sparse_attention(cuda, d, dt, name):
    from gvfdiffusion_amd.sparse import SparseTensor
    from gvfdiffusion_amd.sparse.attention import sparse_scaled_dot_product_attention as spa
    H, worst = 2, []
    coords = _coords("full")
    T, B = coords.shape[0], len(S.SIZES)
    lay = S.layout_of(coords)
    qkv = _qkv(T, H, d, dt, 12)
    st = _sparse(qkv, coords)
    q, k, v = st.unbind(1)
    kv = st.replace(st.feats[:, 1:])
    own = S.sample_spans(lay)
    for form, out in (("qkv", spa(st)), ("q, k, v", spa(q, k, v)), ("q, kv", spa(q, kv))):
        assert isinstance(out, SparseTensor)
        _hold_attention(f"spa({form}) d={d} {name}", out.feats, qkv[:, 0], qkv[:, 1], qkv[:, 2], own, name, worst)
    g = torch.Generator().manual_seed(13)
    Lc, Lq = 50, 40
    ctx = torch.randn((B, Lc, 2, H, d), generator=g).to(dt)
    cross = S.sample_spans(lay, [(b * Lc, (b + 1) * Lc) for b in range(B)])
    out = spa(q, ctx.cuda())
    _hold_attention(f"spa(sparse q, dense kv) d={d} {name}", out.feats, qkv[:, 0], ctx[:, :, 0].reshape(B * Lc, H, d), ctx[:, :, 1].reshape(B * Lc, H, d),
                    cross, name, worst)
    qd = torch.randn((B, Lq, H, d), generator=g).to(dt)
    back = S.sample_spans([(b * Lq, (b + 1) * Lq) for b in range(B)], lay)
    out = spa(qd.cuda(), kv)
    assert out.shape == (B, Lq, H, d)
    _hold_attention(f"spa(dense q, sparse kv) d={d} {name}", out.reshape(B * Lq, H, d), qd.reshape(B * Lq, H, d), qkv[:, 1], qkv[:, 2], back, name, worst)
    print(f"B five call forms d={d} {name}: largest per-group ratio {max(worst):.2f} (m = {S.MARGIN})")


# ---- C. SparseMultiHeadAttention ----------------------------------------------------------------------------------------------------------
MHA_RULES = {"full": dict(kind="full"), "windowed": dict(kind="windowed", window=8, shift=4),
             "serialized": dict(kind="serialized", window=64, shift_sequence=32, shift_window=(0, 0, 0), order="HILBERT"),
             "cross": dict(kind="full")}
CTX_LEN, CTX_CH = 20, 64


def _mha_keys(kind, rms):
    keys = ["attn.to_q.weight", "attn.to_q.bias", "attn.to_kv.weight", "attn.to_kv.bias"] if kind == "cross" else ["attn.to_qkv.weight", "attn.to_qkv.bias"]
    return keys + ["attn.to_out.weight", "attn.to_out.bias"] + (["attn.q_rms_norm.gamma", "attn.k_rms_norm.gamma"] if rms else [])


def _oracle_mha(x, w, ctx, sd, keys, spans, H, precision, old, rms, dtype, round_output=False):
    from oracle import sparse_vae_ref as ref
    leaves = {k: sd[k].to(dtype).requires_grad_() for k in keys}
    xi = x.to(dtype).requires_grad_()
    ci = None if ctx is None else ctx.to(dtype).requires_grad_()
    y = ref.multi_head_attention(xi, spans, leaves, "attn", H, precision, old, rms, context=ci, round_output=round_output)
    wrt = [leaves[k] for k in keys] + [xi] + ([] if ci is None else [ci])
    out = dict(zip([k[5:] for k in keys] + ["x"] + ([] if ci is None else ["ctx"]), torch.autograd.grad((y * w.to(dtype)).sum(), wrt)))
    out["y"] = y.detach()
    return out


@pytest.mark.parametrize("dt,name", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("C", list(S.WIDTHS))
@pytest.mark.parametrize("rms", [False, True], ids=["plain", "qk_rms"])
@pytest.mark.parametrize("old", [True, False], ids=["old_layout", "new_layout"])
@pytest.mark.parametrize("kind", list(MHA_RULES))
def test_multi_head_attention_module(cuda, oracle_lib, kind, old, rms, C, dt, name):
    """The inference forward (fp32 rows under an autocast region of the operand type) and the enable_training() forward under grad: output
    and input gradient (and, for the cross form, the context's) per window; every parameter gradient on the whole tensor at 2 x yardstick."""
    from gvfdiffusion_amd.sparse.attention import SparseMultiHeadAttention
    H, rule = S.WIDTHS[C], MHA_RULES[kind]
    coords = _coords(rule)
    T, B = coords.shape[0], len(S.SIZES)
    lay = S.layout_of(coords)
    sd, x, w = _cached(("state", C), lambda: S.block_state(C, ctx_channels=CTX_CH))
    keys = _mha_keys(kind, rms)
    if kind == "cross":
        ctx = _cached("ctx", lambda: torch.randn((B, CTX_LEN, CTX_CH), generator=torch.Generator().manual_seed(14)))
        ctx_rows = ctx.reshape(B * CTX_LEN, CTX_CH)
        ctx_lay = [(b * CTX_LEN, (b + 1) * CTX_LEN) for b in range(B)]
        spans = S.sample_spans(lay, ctx_lay)
    else:
        ctx = ctx_rows = None
        spans = _spans(oracle_lib, coords, rule)
    groups = S.write_groups(spans)
    r64 = _cached(("mha64", kind, old, rms, C), lambda: _oracle_mha(x, w, ctx_rows, sd, keys, spans, H, "fp32", old, rms, torch.float64))
    yard0 = _oracle_mha(x, w, ctx_rows, sd, keys, spans, H, name, old, rms, torch.float32)["y"]
    # the training route rounds the closing projection's output to the operand type (autocast's placement): so does its yardstick
    yard = _oracle_mha(x, w, ctx_rows, sd, keys, spans, H, name, old, rms, torch.float32, round_output=True)
    kw = dict(type="cross", ctx_channels=CTX_CH) if kind == "cross" else S.module_kwargs(rule)
    m = SparseMultiHeadAttention(C, H, qk_rms_norm=rms, use_old_attn_impl=old, **kw)
    m.load_state_dict({k[5:]: sd[k] for k in keys})
    m = m.cuda()
    st = _sparse(x, coords)
    cg = None if ctx is None else ctx.cuda()
    with torch.no_grad(), torch.autocast("cuda", dtype=dt):
        y0 = m(st) if cg is None else m(st, cg)
    assert y0.feats.dtype == torch.float32
    ratios = {"y (inference)": S.assert_per_group(f"{kind} inference y", y0.feats.cpu(), r64["y"], yard0, groups)}
    m.enable_training(dtype=dt)
    xs = _sparse(x, coords)
    xs.feats.requires_grad_()
    if cg is not None:
        cg = cg.clone().requires_grad_()
    y = m(xs) if cg is None else m(xs, cg)
    assert y.feats.grad_fn is not None
    names, params = zip(*m.named_parameters())
    wrt = list(params) + [xs.feats] + ([] if cg is None else [cg])
    got = dict(zip(names + ("x",) + (() if cg is None else ("ctx",)), torch.autograd.grad((y.feats * w.cuda()).sum(), wrt)))
    ratios["y (training)"] = S.assert_per_group(f"{kind} training y", y.feats.detach().cpu(), r64["y"], yard["y"], groups)
    ratios["dx"] = S.assert_per_group(f"{kind} dx", got["x"].cpu(), r64["x"], yard["x"], groups)
    if cg is not None:
        ratios["dctx"] = S.assert_per_group(f"{kind} dctx", got["ctx"].reshape(B * CTX_LEN, CTX_CH).cpu(), r64["ctx"], yard["ctx"],
                                            [torch.arange(a, b) for a, b in ctx_lay])
    assert set(names) == {k[5:] for k in keys}
    log = []
    for k in names:
        e, ey = R.rel_l2(got[k].cpu(), r64[k]), R.rel_l2(yard[k], r64[k])
        log.append(f"{k} {e:.2e}/{ey:.2e}")
        assert torch.isfinite(got[k]).all() and e <= 2 * ey, f"{kind} old={old} rms={rms} C={C} {name} {k}: rel L2 {e:.3e} > 2 x yardstick {ey:.3e}"
    print(f"C module {kind} old={old} rms={rms} C={C} {name}: per-group ratios", {k: round(v, 2) for k, v in ratios.items()},
          f"(m = {S.MARGIN}) | parameters kernel/yardstick:", "; ".join(log))


# ---- D. SparseTransformerBlock ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt,name", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("C", list(S.WIDTHS))
@pytest.mark.parametrize("i", [0, 1], ids=["even", "odd"])
@pytest.mark.parametrize("mode", S.BLOCK_MODES)
def test_block_rows_per_window(cuda, oracle_lib, mode, i, C, dt, name):
    """Block i of a backbone of each attn_mode (built by build_blocks from block_attn_config) against the oracle over the spans of the
    restated rule: forward_rows, forward_rows_train without grad (and whether the two agree bit for bit: reported, they are different
    launches), forward_rows_train under grad with the input gradient."""
    from types import SimpleNamespace
    from gvfdiffusion_amd.model.sparse_voxel_diffusion.sparse_transformer import build_blocks
    from oracle import sparse_vae_ref as ref
    H, cfg = S.WIDTHS[C], S.block_cfg(mode, C)
    old = C == 128
    rule = ref.block_attn_rule(cfg, i)
    coords = _coords(mode)
    spans = _spans(oracle_lib, coords, rule)
    groups = S.write_groups(spans)
    sd, x, w = _cached(("state", C), lambda: S.block_state(C, ctx_channels=CTX_CH))
    r64 = _cached(("blk64", mode, i, C), lambda: S.oracle_block(x, w, sd, spans, H, "fp32", old, False, torch.float64))
    yard = S.oracle_block(x, w, sd, spans, H, name, old, False, torch.float32)
    blk = build_blocks(SimpleNamespace(num_blocks=2, attn_mode=mode, window_size=cfg["window_size"]), C, H, 4, use_old_attn_impl=old)[i]
    blk.load_state_dict({k: sd[k] for k in S.block_keys(sd, False)})
    blk = blk.cuda()
    st = _sparse(x, coords)
    y0 = blk.forward_rows(x.cuda().clone(), st, dt)
    ratios = {"forward_rows": S.assert_per_group(f"{mode} block {i} forward_rows", y0.cpu(), r64["y"], yard["y"], groups)}
    with torch.no_grad():
        y1 = blk.forward_rows_train(x.cuda(), st, dt, cache={})
    ratios["forward_rows_train (no grad)"] = S.assert_per_group(f"{mode} block {i} forward_rows_train", y1.cpu(), r64["y"], yard["y"], groups)
    same, apart = torch.equal(y0, y1), R.rel_l2(y1, y0)
    xr = x.cuda().requires_grad_()
    y = blk.forward_rows_train(xr, st, dt, cache={})
    dx, = torch.autograd.grad((y * w.cuda()).sum(), [xr])
    assert torch.equal(y.detach(), y1)                                                               # the same launches with and without a graph
    ratios["dx"] = S.assert_per_group(f"{mode} block {i} dx", dx.cpu(), r64["x"], yard["x"], groups)
    print(f"D block {mode} block {i} C={C} {name}: per-group ratios", {k: round(v, 2) for k, v in ratios.items()}, f"(m = {S.MARGIN}) | "
          f"forward_rows == forward_rows_train bit for bit: {same} (relative L2 between them {apart:.2e})")


# ---- E. the backbone ----------------------------------------------------------------------------------------------------------------------
def _vae_cfg(mode):
    return dict(resolution=S.grid_of(mode), in_channels=64, model_channels=128, out_channels=112, latent_channels=8, num_blocks=4, num_heads=2,
                mlp_ratio=4, attn_mode=mode, window_size=8 if mode == "swin" else 64, use_fp16=False, use_old_attn_impl=True, norm_output=True)


def _vae_inputs(mode):
    from gvfdiffusion_amd.model.sparse_voxel_diffusion import SparseTransformerVAE
    cfg = _vae_cfg(mode)
    g = torch.Generator().manual_seed(31)
    sd = {k: torch.randn(v.shape, generator=g) * (v.shape[1] ** -0.5 if v.dim() == 2 else 0.1) for k, v in SparseTransformerVAE(**cfg).state_dict().items()}
    T = sum(S.SIZES)
    return cfg, sd, torch.randn((T, cfg["in_channels"]), generator=g), torch.randn((T, cfg["latent_channels"]), generator=g), \
        torch.randn((T, cfg["out_channels"]), generator=g)


def _oracle_vae(cfg, sd, feats, coords, noise, W, make_spans, precision, dtype):
    """-> dict mean, logvar, decode (of the float64 mean handed in as `zin`), out (the training forward's) and dfeats of sum(out * W) / T + kl"""
    from oracle import sparse_vae_ref as ref
    leaves = {k: v.to(dtype) for k, v in sd.items()}
    x = feats.to(dtype).requires_grad_()
    mean, logvar = ref.encode_spans(leaves, cfg, x, coords, make_spans, precision)
    z = mean + torch.exp(0.5 * logvar) * noise.to(dtype)
    out = ref.decode_spans(leaves, cfg, z, coords, make_spans, precision)
    kl = 0.5 * torch.mean(mean.pow(2) + logvar.exp() - logvar - 1)
    g, = torch.autograd.grad((out * W.to(dtype)).sum() / feats.shape[0] + kl, [x])
    return dict(mean=mean.detach(), logvar=logvar.detach(), out=out.detach(), dfeats=g)


@pytest.mark.parametrize("dt,name", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("mode", S.BLOCK_MODES)
def test_backbone_every_attn_mode(cuda, oracle_lib, mode, dt, name):
    """SparseTransformerVAE, 128 channels, 4 + 4 blocks (shift_order visits all four curves): encode mean / logvar and decode on the
    inference path, forward under enable_training() with the gradient at the input features; per sample and per chunk of 16 rows."""
    from gvfdiffusion_amd.model.sparse_voxel_diffusion import SparseTransformerVAE
    from oracle import sparse_vae_ref as ref
    coords = _coords(mode)
    cfg, sd, feats, noise, W = _cached(("vae", mode), lambda: _vae_inputs(mode))
    groups = S.chunk_groups(S.layout_of(coords))
    make = lambda rule: _spans(oracle_lib, coords, rule)   # noqa: E731

    def decode_of(z, precision):
        with torch.no_grad():
            return ref.decode_spans(sd if precision != "fp64" else {k: v.double() for k, v in sd.items()}, cfg, z, coords, make,
                                    "fp32" if precision == "fp64" else precision)
    r64 = _cached(("vae64", mode), lambda: _oracle_vae(cfg, sd, feats, coords, noise, W, make, "fp32", torch.float64))
    zin = r64["mean"].float()                                                                      # what the inference decode is fed
    d64 = _cached(("dec64", mode), lambda: decode_of(zin.double(), "fp64"))
    yard = _oracle_vae(cfg, sd, feats, coords, noise, W, make, name, torch.float32)
    dyard = decode_of(zin, name)
    m = SparseTransformerVAE(**cfg)
    m.load_state_dict(sd, strict=True)
    m = m.cuda().set_compute_dtype(dt)
    x = _sparse(feats, coords)
    z, mean, logvar = m.encode(x, sample_posterior=False, return_raw=True)
    y = m.decode(_sparse(zin, coords))
    ratios = {"mean": S.assert_per_group(f"{mode} mean", mean.cpu(), r64["mean"], yard["mean"], groups),
              "logvar": S.assert_per_group(f"{mode} logvar", logvar.cpu(), r64["logvar"], yard["logvar"], groups),
              "decode": S.assert_per_group(f"{mode} decode", y.feats.cpu(), d64, dyard, groups)}
    m.enable_training(dtype=dt)
    xs = _sparse(feats, coords)
    xs.feats.requires_grad_()
    loss, out = R.model_loss(m, xs, noise.cuda(), W.cuda())
    scale = 1024.0 if dt == torch.float16 else 1.0
    g, = torch.autograd.grad(loss * scale, [xs.feats])
    ratios["forward"] = S.assert_per_group(f"{mode} training forward", out.feats.detach().cpu(), r64["out"], yard["out"], groups)
    ratios["dfeats"] = S.assert_per_group(f"{mode} dfeats", (g / scale).cpu(), r64["dfeats"], yard["dfeats"], groups)
    print(f"E backbone {mode} {name}: per-group ratios", {k: round(v, 2) for k, v in ratios.items()}, f"(m = {S.MARGIN}, {len(groups)} groups)")


# ---- F. the plan cache --------------------------------------------------------------------------------------------------------------------
def test_plan_cache_follows_the_coordinates(cuda, oracle_lib):
    from gvfdiffusion_amd.sparse.attention import (sparse_windowed_scaled_dot_product_self_attention as win_attn,
                                                   sparse_serialized_scaled_dot_product_self_attention as ser_attn, SerializeMode)
    from gvfdiffusion_amd.model.sparse_voxel_diffusion import SparseTransformerBlock
    H, d, dt, name = 2, 64, torch.bfloat16, "bf16"
    coords, other = _coords("full"), S.voxels(16, seed=77)
    assert S.layout_of(coords) == S.layout_of(other) and not torch.equal(coords, other)
    T = coords.shape[0]
    rw, rs = WIN_CFG[1], dict(kind="serialized", window=64, shift_sequence=32, shift_window=(0, 0, 0), order="Z_ORDER")
    run = {"windowed": lambda t: win_attn(t, 8, (4, 4, 4)), "serialized": lambda t: ser_attn(t, 64, SerializeMode.Z_ORDER, 32, (0, 0, 0))}
    worst = []
    for kind, rule in (("windowed", rw), ("serialized", rs)):
        a, b = _qkv(T, H, d, dt, 41), _qkv(T, H, d, dt, 42)
        st = _sparse(a, coords)
        out = run[kind](st)
        plans = dict(st.get_spatial_cache())
        assert len(plans) == 1
        plan = next(iter(plans.values()))
        # replace(feats): the same plan object, and the result of the new features
        st2 = st.replace(b.cuda())
        out2 = run[kind](st2)
        assert next(iter(st2.get_spatial_cache().values())) is plan and len(st2.get_spatial_cache()) == 1
        own = S.spans_of_rule(oracle_lib, coords, rule)
        _hold_attention(f"cache {kind} first", out.feats, a[:, 0], a[:, 1], a[:, 2], own, name, worst)
        _hold_attention(f"cache {kind} replace(feats)", out2.feats, b[:, 0], b[:, 1], b[:, 2], own, name, worst)
        # the same layout sizes on other coordinates: a tensor of its own, and replace(feats, coords)
        theirs = S.spans_of_rule(oracle_lib, other, rule)
        for tag, st3 in (("new tensor", _sparse(b, other)), ("replace(feats, coords)", st.replace(b.cuda(), other.cuda()))):
            out3 = run[kind](st3)
            plan3 = next(iter(st3.get_spatial_cache().values()))
            assert plan3 is not plan and not (plan3[0].shape == plan[0].shape and torch.equal(plan3[0], plan[0]))
            _hold_attention(f"cache {kind} {tag}", out3.feats, b[:, 0], b[:, 1], b[:, 2], theirs, name, worst)
        assert next(iter(st.get_spatial_cache().values())) is plan and len(st.get_spatial_cache()) == 1       # the first tensor's is untouched
    # a block twice on one tensor (the second run reads the cached plan): equal bits
    sd, x, w = _cached(("state", 128), lambda: S.block_state(128, ctx_channels=CTX_CH))
    for rule in (rw, rs):
        blk = SparseTransformerBlock(128, num_heads=2, modulated=False, use_old_attn_impl=True, **S.module_kwargs(rule))
        blk.load_state_dict({k: sd[k] for k in S.block_keys(sd, False)})
        blk = blk.cuda()
        st = _sparse(x, coords)
        y1 = blk.forward_rows(x.cuda().clone(), st, dt)
        assert len(st.get_spatial_cache()) == 1
        y2 = blk.forward_rows(x.cuda().clone(), st, dt)
        y3 = blk(st).feats
        assert torch.equal(y1, y2) and torch.equal(y1, y3) and len(st.get_spatial_cache()) == 1
    print(f"F cache: largest per-group ratio {max(worst):.2f} (m = {S.MARGIN})")
