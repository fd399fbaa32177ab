"""The ragged attention backward (gvf_attn_varlen_bwd through ops/attention_grad.py::attention_varlen, the seam
sparse/attention/full_attn.py and SparseMultiHeadAttention.enable_training) on an MI355X.

Every gradient is compared with the float64 formula of tests/attn_bwd_ref.py looped over the sequences (tests/attn_varlen_ref.py) on the
same 16-bit operands, by the two measures of tests/test_attn_bwd_gpu.py -- whole-tensor relative L2 and worst 32-row block -- taken per
sequence (a misplaced or dropped sequence is averaged away in a whole-tensor figure) and over the whole packed tensor.  Bar of each: twice
what the yardstick (the fp32 composition with the kernel's rounding points) gives on the same rows.  dQ and dK of a sequence with ONE key
are zero in exact arithmetic and are held element by element to the floor derived in tests/test_attn_bwd_gpu.py.

Module bars (test_module_gradients_against_fp64): rel L2 of every parameter / input gradient from the fp64 torch composition on the CPU,
at most twice the same composition's deviation under CPU autocast of the matching type."""
import pytest
import torch
import torch.nn.functional as F

import attn_bwd_ref as R
import attn_varlen_ref as V
from gvfdiffusion_amd.ops import attention_grad as AG, dit_ops
from gvfdiffusion_amd.sparse import SparseTensor
from gvfdiffusion_amd.sparse.attention import SerializeMode, SparseMultiHeadAttention
from gvfdiffusion_amd.sparse.attention.full_attn import sparse_scaled_dot_product_attention as sparse_sdpa

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]
H = 2
SELF_LENS = [1, 31, 32, 33, 127, 128, 129, 218, 260]
CROSS_Q = [40, 0, 130, 5, 1024]
CROSS_K = [300, 64, 0, 33, 64]
CASES = {"self": (SELF_LENS, SELF_LENS, 21), "cross": (CROSS_Q, CROSS_K, 22)}


def _name(dt):
    return str(dt)[6:]


def _floor(q, k, v, do, scale):
    """Elementwise bounds of dQ and dK of one sequence [1, L, H, C] whose keys are all equal (here: one key); see tests/test_attn_bwd_gpu.py."""
    qd, kd, vd, dod = (t.double() for t in (q, k, v, do))
    Lk = k.shape[1]
    a = (dod.abs()[:, :, None] * vd.abs()[:, None]).sum(-1).amax(dim=2)
    fq = 2.0 ** -20 * scale * a[..., None] * kd.abs().amax(dim=1, keepdim=True)
    fk = 2.0 ** -20 * scale * (a[..., None] * qd.abs()).sum(dim=1, keepdim=True).expand(-1, Lk, -1, -1) / Lk
    return fq, fk


def _hold(label, g, r, y, lens=None, skip=()):
    """Both measures of g against r at most twice the yardstick y's: over the whole packed tensor and, with lens, per sequence (but `skip`)."""
    parts = [("all", g[None], r[None], y[None])]
    if lens is not None:
        parts += [(f"seq {i} ({gs.shape[1]} rows)", gs, rs, ys) for (i, gs, rs), (_, ys, _) in zip(V.per_sequence(g, r, lens), V.per_sequence(y, r, lens))
                  if i not in skip]
    for what, gs, rs, ys in parts:
        e, ey = R.rel_l2(gs, rs), R.rel_l2(ys, rs)
        b, by = R.worst_block(gs, rs), R.worst_block(ys, rs)
        print(f"{label} {what}: rel L2 hip {e:.2e} yardstick {ey:.2e}; worst block hip {b:.2e} yardstick {by:.2e}")
        assert e <= 2 * ey, (label, what, e, ey)
        assert b <= 2 * by, (label, what, b, by)


def _is_plus_zero(t):
    return not bool(t.contiguous().view(torch.int16).any())


_REF = {}


@pytest.fixture(scope="module", autouse=True)
def _release_shared_references():
    yield
    _REF.clear()


def _case(cuda, case, C, dt):
    """Operands, cu_seqlens, the fp64 reference and the yardstick of one configuration: computed once, shared, left unchanged."""
    key = (case, C, dt)
    if key not in _REF:
        q_lens, k_lens, seed = CASES[case]
        q, k, v, do = V.make_packed(q_lens, k_lens, H, C, dt, device=cuda, seed=seed)
        scale = C ** -0.5
        _REF[key] = dict(q=q, k=k, v=v, do=do, q_lens=q_lens, k_lens=k_lens, scale=scale, cu_q=V.cu(q_lens, cuda), cu_k=V.cu(k_lens, cuda),
                         ref=V.packed_grads64(q, k, v, do, q_lens, k_lens, scale), yd=V.packed_yardstick(q, k, v, do, q_lens, k_lens, scale, dt))
    return _REF[key]


def _run(c, scale=None):
    q, k, v = (c[n].detach().clone().requires_grad_(True) for n in "qkv")
    out = AG.attention_varlen(q, k, v, c["cu_q"], c["cu_k"], max(c["q_lens"]), max(c["k_lens"]), scale)
    out.backward(c["do"])
    return out.detach(), q.grad, k.grad, v.grad


@pytest.mark.parametrize("dt", DTYPES, ids=_name)
@pytest.mark.parametrize("C", [32, 64])
@pytest.mark.parametrize("case", list(CASES))
def test_ragged_gradients_against_fp64(cuda, case, C, dt):
    c = _case(cuda, case, C, dt)
    q_lens, k_lens = c["q_lens"], c["k_lens"]
    if case == "cross":     # 3 key blocks x 10 problems against 32 query tiles: the key sweep is split, its partials are in the workspace
        stats = 2 * ((4 * H * sum(q_lens) + 255) // 256 * 256)
        assert AG.varlen_workspace_bytes(len(q_lens), sum(q_lens), sum(k_lens), max(q_lens), max(k_lens), H, C) >= stats + 2 * 2 * 4 * H * sum(k_lens) * C
    out, dq, dk, dv = _run(c)
    with torch.no_grad():
        plain = AG.attention_varlen(c["q"], c["k"], c["v"], c["cu_q"], c["cu_k"], max(q_lens), max(k_lens))
    assert torch.equal(plain, out), "forward under grad differs from the no-grad forward"
    label = f"{case} d {C} {_name(dt)}"
    _hold(f"{label} out", out, c["ref"][0], c["yd"][0])
    for g in (dq, dk, dv):
        assert g.dtype == dt and not torch.isnan(g).any()
    qb, kb = V.bounds(q_lens), V.bounds(k_lens)
    one_key = [i for i, (a, b) in enumerate(kb) if b - a == 1 and qb[i][1] > qb[i][0]]
    # sequences with one key: dQ, dK exact zeros, held to the floor; they stay in the whole-tensor figure and leave the per-sequence ones
    for i in one_key:
        (a, b), (s, e) = qb[i], kb[i]
        fq, fk = _floor(c["q"][None, a:b], c["k"][None, s:e], c["v"][None, s:e], c["do"][None, a:b], c["scale"])
        assert bool((dq[None, a:b].double().abs() <= fq).all()) and bool((dk[None, s:e].double().abs() <= fk).all()), (label, "one key", i)
    _hold(f"{label} dq", dq, c["ref"][1], c["yd"][1], q_lens, skip=one_key)
    _hold(f"{label} dk", dk, c["ref"][2], c["yd"][2], k_lens, skip=one_key)
    _hold(f"{label} dv", dv, c["ref"][3], c["yd"][3], k_lens)
    # empty sequences: queries without keys get dq = +0 (and zero output rows), keys without queries dk = dv = +0
    for (a, b), (s, e) in zip(qb, kb):
        if e == s and b > a:
            assert _is_plus_zero(dq[a:b]) and _is_plus_zero(out[a:b])
        if b == a and e > s:
            assert _is_plus_zero(dk[s:e]) and _is_plus_zero(dv[s:e])


def _banded(t, band=40):
    """t [T, H, C] in the middle of a NaN-filled buffer: (view of the middle, whole buffer)."""
    buf = torch.full((t.shape[0] + 2 * band,) + tuple(t.shape[1:]), float("nan"), dtype=t.dtype, device=t.device)
    buf[band:band + t.shape[0]] = t
    return buf[band:band + t.shape[0]], buf


@pytest.mark.parametrize("dt", DTYPES, ids=_name)
@pytest.mark.parametrize("C", [32, 64])
@pytest.mark.parametrize("case", list(CASES))
def test_guard_bands_nan_workspace_and_equal_bits(cuda, case, C, dt):
    c = _case(cuda, case, C, dt)
    q_lens, k_lens = c["q_lens"], c["k_lens"]
    mq, mk = max(q_lens), max(k_lens)
    first = _run(c)
    band = 40
    ins = {n: _banded(c[n], band) for n in ("q", "k", "v", "do")}
    out_v, out_buf = _banded(torch.zeros_like(c["q"]), band)
    _st3 = AG._st3
    dit_ops.attention_varlen(ins["q"][0], ins["k"][0], ins["v"][0], out_v, c["cu_q"], c["cu_k"], mq, mk, H, _st3(ins["q"][0]), _st3(ins["k"][0]),
                             _st3(ins["v"][0]), _st3(out_v), scale=c["scale"], head_dim=C)
    assert torch.equal(out_v, first[0])
    grads = [_banded(torch.zeros_like(c[n]), band) for n in ("q", "k", "v")]
    for gv, _ in grads:
        gv.fill_(float("nan"))                                # every gradient row has to be written
    nbytes = AG.varlen_workspace_bytes(len(q_lens), sum(q_lens), sum(k_lens), mq, mk, H, C)
    ws = torch.full(((nbytes + 3) // 4,), float("nan"), dtype=torch.float32, device=cuda).view(torch.uint8)
    got = AG.attention_varlen_backward(ins["q"][0], ins["k"][0], ins["v"][0], out_v, ins["do"][0], c["cu_q"], c["cu_k"], mq, mk, c["scale"],
                                       workspace=ws, grads=tuple(g for g, _ in grads))
    for (gv, buf), g, f in zip(grads, got, first[1:]):
        assert g.data_ptr() == gv.data_ptr()
        assert not torch.isnan(gv).any(), "a gradient row was left unwritten, or NaN from the workspace reached it"
        assert torch.isnan(buf[:band]).all() and torch.isnan(buf[-band:]).all(), "a gradient guard band was written"
        assert torch.equal(gv, f), "second call (caller-owned buffers, NaN workspace): other bits"
    for _, buf in list(ins.values()) + [(None, out_buf)]:
        assert torch.isnan(buf[:band]).all() and torch.isnan(buf[-band:]).all()
    # the same call on a second stream, while this stream runs another problem
    other = _case(cuda, "self" if case == "cross" else "cross", C, dt)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        busy = AG.attention_varlen_backward(c["q"], c["k"], c["v"], first[0], c["do"], c["cu_q"], c["cu_k"], mq, mk, c["scale"])
    _run(other)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for a, b in zip(first[1:], busy):
        assert torch.equal(a, b), "second stream: other bits"


def test_totals_of_zero_need_no_launch(cuda):
    cu0, cu = V.cu([0, 0], cuda), V.cu([3, 4], cuda)
    for tq, tk, cq, ck in ((0, 7, cu0, cu), (7, 0, cu, cu0)):
        q = torch.randn((tq, H, 32), device=cuda).half().requires_grad_(True)
        k = torch.randn((tk, H, 32), device=cuda).half().requires_grad_(True)
        v = torch.randn((tk, H, 32), device=cuda).half().requires_grad_(True)
        out = AG.attention_varlen(q, k, v, cq, ck, 4 if tq else 0, 4 if tk else 0)
        assert out.shape == q.shape and not out.any()
        out.backward(torch.ones_like(out))
        for t in (q, k, v):
            assert t.grad is not None and t.grad.shape == t.shape and not t.grad.any()
    q = torch.randn((7, H, 48), device=cuda).half()
    with pytest.raises(NotImplementedError):
        AG.attention_varlen(q, q, q, cu, cu, 4, 4)
    q = q[..., :32].contiguous()
    with pytest.raises(ValueError):
        AG.attention_varlen(q, q[:, :1], q[:, :1], cu, cu, 4, 4)


# ---- the seam ------------------------------------------------------------------------------------------------------------------------------
def _coords(lens, device):
    """Distinct voxels of a 16^3 grid per batch element."""
    g = torch.Generator().manual_seed(sum(lens))
    rows = []
    for b, n in enumerate(lens):
        idx = torch.randperm(16 ** 3, generator=g)[:n]
        rows.append(torch.stack([torch.full((n,), b), idx // 256, (idx // 16) % 16, idx % 16], dim=1))
    return torch.cat(rows).int().to(device)


@pytest.mark.parametrize("leaves", ["fp32_autocast_fp16", "float16", "bfloat16"])
@pytest.mark.parametrize("C", [32, 64])
def test_the_sparse_seam_carries_gradients(cuda, C, leaves):
    dt = torch.bfloat16 if leaves == "bfloat16" else torch.float16
    leaf_dt = torch.float32 if leaves.startswith("fp32") else dt
    q_lens, k_lens, Lk = [150, 37, 129], [150, 37, 129], 40
    coords = _coords(q_lens, cuda)
    scale = C ** -0.5

    def leaf(t):
        return t.to(leaf_dt).detach().clone().requires_grad_(True)          # (16-bit values: the cast to fp32 and back is exact)

    def call(*args):
        with torch.autocast("cuda", dtype=torch.float16, enabled=leaf_dt == torch.float32):
            return sparse_sdpa(*args)

    def feats(o):
        return o.feats if isinstance(o, SparseTensor) else o.reshape(-1, *o.shape[2:])

    q, k, v, do = V.make_packed(q_lens, k_lens, H, C, dt, device=cuda, seed=31)
    ref, yd = V.packed_grads64(q, k, v, do, q_lens, k_lens, scale), V.packed_yardstick(q, k, v, do, q_lens, k_lens, scale, dt)
    # (qkv): on the parent commit the output had no grad_fn and qkv.grad stayed None
    qkv = leaf(torch.stack([q, k, v], dim=1))
    out = call(SparseTensor(qkv, coords))
    assert out.feats.requires_grad and out.feats.dtype == leaf_dt
    out.feats.backward(do.to(leaf_dt))
    assert qkv.grad is not None and qkv.grad.shape == qkv.shape and qkv.grad.dtype == leaf_dt
    for i, name in enumerate(("dq", "dk", "dv")):
        _hold(f"(qkv) {leaves} d {C} {name}", qkv.grad[:, i], ref[1 + i], yd[1 + i], q_lens)
    with torch.no_grad():
        assert torch.equal(call(SparseTensor(qkv, coords)).feats, out.feats), "output under grad differs from the no-grad output"
    # (q, k, v) sparse; then only one of them requiring grad
    for who in (None, 0, 1, 2):
        ls = [leaf(t) if who in (None, i) else t.to(leaf_dt) for i, t in enumerate((q, k, v))]
        call(*(SparseTensor(t, coords) for t in ls)).feats.backward(do.to(leaf_dt))
        for i, name in enumerate(("dq", "dk", "dv")):
            if who in (None, i):
                _hold(f"(q, k, v) needs {who} {leaves} d {C} {name}", ls[i].grad, ref[1 + i], yd[1 + i], q_lens)
            else:
                assert ls[i].grad is None
    # (q sparse, kv dense) and (q dense, kv sparse): the dense side has equal lengths
    for q_dense in (False, True):
        ql = [Lk] * 3 if q_dense else q_lens
        kl = k_lens if q_dense else [Lk] * 3
        q2, k2, v2, do2 = V.make_packed(ql, kl, H, C, dt, device=cuda, seed=32 + q_dense)
        ref2, yd2 = V.packed_grads64(q2, k2, v2, do2, ql, kl, scale), V.packed_yardstick(q2, k2, v2, do2, ql, kl, scale, dt)
        qq, kv = leaf(q2), leaf(torch.stack([k2, v2], dim=1))
        if q_dense:
            o = call(qq.reshape(3, Lk, H, C), SparseTensor(kv, coords))
        else:
            o = call(SparseTensor(qq, coords), kv.reshape(3, Lk, 2, H, C))
        feats(o).backward(do2.to(leaf_dt))
        _hold(f"(q, kv) q_dense {q_dense} {leaves} d {C} dq", qq.grad, ref2[1], yd2[1], ql)
        _hold(f"(q, kv) q_dense {q_dense} {leaves} d {C} dk", kv.grad[:, 0], ref2[2], yd2[2], kl)
        _hold(f"(q, kv) q_dense {q_dense} {leaves} d {C} dv", kv.grad[:, 1], ref2[3], yd2[3], kl)


def _rms(t, gamma, C):
    return F.normalize(t, dim=-1) * gamma * C ** 0.5


@pytest.mark.parametrize("dt", DTYPES, ids=_name)
@pytest.mark.parametrize("C", [32, 64])
def test_the_seam_with_gains(cuda, C, dt):
    """packed_varlen_attention with QK-RMSNorm gains under grad: rmsnorm_heads in front of the ragged operator.  Reference: the norm and
    the attention in float64; yardstick: the norm in fp32 rounded to the operand type, the attention yardstick, the norm's fp32 backward."""
    from gvfdiffusion_amd.sparse.attention.full_attn import packed_varlen_attention
    q_lens = k_lens = [100, 33, 161]
    q, k, v, do = V.make_packed(q_lens, k_lens, H, C, dt, device=cuda, seed=41)
    g = torch.Generator().manual_seed(42)
    gq, gk = ((1.0 + 0.2 * torch.randn((H, C), generator=g)).to(cuda) for _ in range(2))
    scale = C ** -0.5
    ls = [t.detach().clone().requires_grad_(True) for t in (q, k, v)]
    gs = [t.detach().clone().requires_grad_(True) for t in (gq, gk)]
    out = packed_varlen_attention(ls[0], ls[1], ls[2], q_lens, k_lens, gs[0], gs[1])
    out.backward(do)

    def through_norm(cd, round_to):
        q_, k_ = (t.to(cd).detach().requires_grad_(True) for t in (q, k))
        a, b = (t.to(cd).detach().requires_grad_(True) for t in (gq, gk))
        qn, kn = _rms(q_, a, C), _rms(k_, b, C)
        q16, k16 = (qn.detach().to(round_to), kn.detach().to(round_to)) if round_to is not None else (qn.detach(), kn.detach())
        if round_to is None:
            o, dqn, dkn, dv = V.packed_grads64(q16, k16, v, do, q_lens, k_lens, scale)
        else:
            o, dqn, dkn, dv = V.packed_yardstick(q16, k16, v, do, q_lens, k_lens, scale, round_to)
        dq, da = torch.autograd.grad(qn, (q_, a), dqn.to(cd))
        dk, db = torch.autograd.grad(kn, (k_, b), dkn.to(cd))
        if round_to is not None:
            dq, dk = dq.to(round_to), dk.to(round_to)
        return o, dq, dk, dv, da, db

    ref, yd = through_norm(torch.float64, None), through_norm(torch.float32, dt)
    got = (out.detach(), ls[0].grad, ls[1].grad, ls[2].grad, gs[0].grad, gs[1].grad)
    for name, g_, r_, y_ in zip(("out", "dq", "dk", "dv", "dgamma_q", "dgamma_k"), got, ref, yd):
        lens = None if name.startswith("dgamma") or name == "out" else q_lens
        if name.startswith("dgamma"):
            g_, r_, y_ = g_[:, None], r_[:, None], y_[:, None]                # [H, 1, C] -> the measures' [1, L, H, C] view below
        _hold(f"gains d {C} {_name(dt)} {name}", g_, r_, y_, lens)


# ---- the module -----------------------------------------------------------------------------------------------------------------------------
MODULES = {
    "self_full_norm": dict(attn_mode="full", qk_rms_norm=True),
    "self_full_old_layout": dict(attn_mode="full", use_old_attn_impl=True),
    "self_windowed_old_layout_norm": dict(attn_mode="windowed", window_size=8, shift_window=(4, 4, 4), qk_rms_norm=True, use_old_attn_impl=True),
    "self_serialized": dict(attn_mode="serialized", window_size=32, serialize_mode=SerializeMode.Z_ORDER, shift_sequence=0, shift_window=(0, 0, 0)),
    "cross_dense_ctx_norm": dict(type="cross", ctx_channels=32, qk_rms_norm=True),
    "cross_sparse_ctx_old_layout": dict(type="cross", ctx_channels=64, use_old_attn_impl=True),
}


def _compose(m, P, xf, cf, seq, kv_seq, fwd, bwd):
    """SparseMultiHeadAttention.forward as a torch composition on the parameters P (a dict by name) in their own type."""
    Hh, c = m.num_heads, m.channels // m.num_heads

    def lin(name, t):
        return F.linear(t, P[name + ".weight"], P[name + ".bias"])

    def split(rows, parts):
        if m.use_old_attn_impl:
            return rows.reshape(rows.shape[0], Hh, parts, c).unbind(dim=2)
        return rows.reshape(rows.shape[0], parts, Hh, c).unbind(dim=1)

    if m._type == "self":
        q, k, v = split(lin("to_qkv", xf), 3)
    else:
        q = lin("to_q", xf).reshape(-1, Hh, c)
        k, v = split(lin("to_kv", cf), 2)
    if m.qk_rms_norm:
        wide = torch.float64 if xf.dtype == torch.float64 else torch.float32
        q = _rms(q.to(wide), P["q_rms_norm.gamma"], c).to(q.dtype)
        k = _rms(k.to(wide), P["k_rms_norm.gamma"], c).to(k.dtype)
    if fwd is not None:
        q, k, v = q[fwd], k[fwd], v[fwd]
    outs = []
    for (a, b), (s, e) in zip(V.bounds(seq), V.bounds(kv_seq)):
        p = torch.softmax(torch.einsum("qhc,khc->hqk", q[a:b], k[s:e]) * c ** -0.5, dim=-1)
        outs.append(torch.einsum("hqk,khc->qhc", p.to(v.dtype), v[s:e]))
    out = torch.cat(outs)
    if bwd is not None:
        out = out[bwd]
    return lin("to_out", out.reshape(out.shape[0], -1))


@pytest.mark.parametrize("dt", DTYPES, ids=_name)
@pytest.mark.parametrize("cfg", list(MODULES), ids=str)
def test_module_gradients_against_fp64(cuda, cfg, dt):
    kw = MODULES[cfg]
    with torch.random.fork_rng(devices=[]), torch.no_grad():   # seeded parameters; the process's generator is left as it was
        torch.manual_seed(3)
        m = SparseMultiHeadAttention(64, 2, **kw)
        for n, p in m.named_parameters():
            if n.endswith("gamma"):
                p.mul_(1.0 + 0.2 * torch.randn_like(p))
            elif n.endswith("bias"):
                p.add_(0.1 * torch.randn_like(p))
    lens = [300, 77]
    coords = _coords(lens, "cpu")
    g = torch.Generator().manual_seed(4)
    xf = torch.randn((sum(lens), 64), generator=g)
    dy = torch.randn((sum(lens), 64), generator=g)
    cross = kw.get("type") == "cross"
    cf = c_lens = None
    if cross:
        c_lens = [20, 20] if kw["ctx_channels"] == 32 else [45, 130]
        cf = torch.randn((sum(c_lens), kw["ctx_channels"]), generator=g)
    mg = SparseMultiHeadAttention(64, 2, **kw).to(cuda)
    mg.load_state_dict(m.state_dict())
    mg.enable_training(dtype=dt)
    xg = xf.to(cuda).requires_grad_(True)
    x = SparseTensor(xg, coords.to(cuda))
    # token orders from the module's own index builder (its Morton / Hilbert codes are computed on the device)
    fwd, bwd, seq = mg._token_order(x, lens)
    fwd, bwd = (None if t is None else t.cpu().long() for t in (fwd, bwd))
    kv_seq = c_lens if cross else seq

    def cpu_grads(mode):
        wide = torch.float64 if mode is None else torch.float32
        P = {n: p.detach().to(wide).requires_grad_(True) for n, p in m.named_parameters()}
        x_, c_ = xf.to(wide).clone().requires_grad_(True), (cf.to(wide).clone().requires_grad_(True) if cross else None)
        with torch.autocast("cpu", dtype=mode if mode is not None else torch.bfloat16, enabled=mode is not None):
            y = _compose(m, P, x_, c_, seq, kv_seq, fwd, bwd)
        y.backward(dy.to(y.dtype))
        out = {n: p.grad for n, p in P.items()}
        out["x"] = x_.grad
        if cross:
            out["context"] = c_.grad
        return y.detach(), out

    y64, g64 = cpu_grads(None)
    y16, g16 = cpu_grads(dt)

    ctx = cg = None
    if cross:
        cg = cf.to(cuda).requires_grad_(True)
        ctx = cg.reshape(2, 20, 32) if kw["ctx_channels"] == 32 else SparseTensor(cg, _coords(c_lens, cuda))
    y = mg(x, ctx)
    assert isinstance(y, SparseTensor) and y.feats.dtype == torch.float32 and y.feats.requires_grad
    y.feats.backward(dy.to(cuda))
    got = {n: p.grad for n, p in mg.named_parameters()}
    got["x"] = xg.grad
    if cross:
        got["context"] = cg.grad
    e, bar = R.rel_l2(y.feats.detach().cpu(), y64), R.rel_l2(y16, y64)
    print(f"module {cfg} {_name(dt)} output: rel L2 hip {e:.2e} cpu autocast {bar:.2e} ({e / bar:.2f}x)")
    assert e <= 2 * bar
    bad = []
    for n in g64:
        assert got[n] is not None, f"{n}: no gradient"
        assert got[n].dtype == torch.float32 and torch.isfinite(got[n]).all(), n
        e, bar = R.rel_l2(got[n].cpu(), g64[n]), R.rel_l2(g16[n], g64[n])
        print(f"module {cfg} {_name(dt)} {n}: grad rel L2 from fp64: hip {e:.2e} cpu autocast {bar:.2e} ({e / bar:.2f}x)")
        if not e <= 2 * bar:
            bad.append((n, e, bar))
    assert not bad, bad
    # with the switch off, and under no_grad with it on, forward is the inference route: same bits, no graph
    with torch.no_grad():
        on = mg(x, ctx).feats
    mg.enable_training(False)
    with torch.no_grad():
        off = mg(x, ctx).feats
    assert torch.equal(on, off) and not off.requires_grad


def test_module_refuses_channel_counts_the_projection_kernels_do_not_take(cuda):
    m = SparseMultiHeadAttention(64, 2, type="cross", ctx_channels=48).to(cuda).enable_training()
    x = SparseTensor(torch.randn((50, 64), device=cuda), _coords([30, 20], cuda))
    with pytest.raises(ValueError):
        m(x, torch.randn((2, 8, 48), device=cuda))
