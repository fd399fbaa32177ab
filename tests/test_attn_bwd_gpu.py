"""The attention backward (csrc/attn_bwd.hip through ops/attention_grad.py and the seam model/attention/full_attn.py) on an MI355X.

Every gradient is compared with the float64 formula of tests/attn_bwd_ref.py on the same 16-bit operands, by two measures: the
whole-tensor relative L2 and the worst 32-row block of one (sequence, head) problem.  The bar of each measure is twice what the
yardstick -- an fp32 torch composition with the kernel's rounding points, computed here on the same inputs -- gives: room for another
summation order, not for another algorithm.

The floor.  A gradient that is zero in exact arithmetic has no relative error, so it is held element by element.  With one key (or
with all keys and all values identical) p = 1 / Lk for every key and dP_k - delta = dO . v - dO . O with O = v exactly (a mean of equal
16-bit numbers rounds back to that number), i.e. the difference of two fp32 evaluations of the same D-long dot product in different
orders: at most 2^-20 sum_d |dO_d v_d| for D <= 64 (16 units of 2^-24 against a random-walk error of about sqrt(D) of them).  Hence
    |dQ[q, d]| <= 2^-20 scale sum_d' |dO[q, d'] v[d']| |k[d]|        (sum_k p_k = 1)
    |dK[k, d]| <= 2^-20 scale sum_q p_k sum_d' |dO[q, d'] v[d']| |q[q, d]|      (its mirror image, p_k = 1 / Lk)."""
import pytest
import torch
from torch import nn

import attn_bwd_ref as R
from gvfdiffusion_amd import training
from gvfdiffusion_amd.model.attention import scaled_dot_product_attention as sdpa
from gvfdiffusion_amd.model.attention.modules import MultiHeadRMSNorm
from gvfdiffusion_amd.ops import attention_grad as AG

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]
# (N, Lq, Lk, H, head_dim)
MODEL_SHAPES = {
    "dit_spatial": (24, 512, 512, 16, 32),
    "dit_temporal": (512, 24, 24, 16, 32),
    "image_cross": (4, 512, 1370, 16, 32),
    "static_cross": (2, 512, 4096, 16, 32),
    "vae_self": (2, 512, 512, 12, 64),
    "vae_decoder_cross": (1, 8192, 512, 12, 64),
}
_EDGE = [1, 31, 32, 33, 63, 64, 65, 127, 129, 257]
EDGE_PAIRS = sorted({(a, a) for a in _EDGE} | {(_EDGE[i], _EDGE[(i + 3) % 10]) for i in range(10)} | {(_EDGE[i], _EDGE[(i + 7) % 10]) for i in range(10)})


def _name(dt):
    return str(dt)[6:]


def _ratio(a, b):
    """a / b for the printed lines; an exact yardstick (one query and one key: dV = dO) has no ratio."""
    return f"{a / b:.2f}x" if b > 0 else ("equal" if a == b else "inf")


def _run(q, k, v, do, scale=None):
    """out and the three gradients of the operator on detached copies of the operands."""
    q, k, v = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    out = AG.attention(q, k, v, scale)
    out.backward(do)
    return out.detach(), q.grad, k.grad, v.grad


def _floor(q, k, v, do, scale):
    """Elementwise bounds of dQ and dK where they are zero in exact arithmetic (module docstring); fp64 [N, L, H, C]."""
    qd, kd, vd, dod = (t.double() for t in (q, k, v, do))
    Lk = k.shape[1]
    a = (dod.abs()[:, :, None] * vd.abs()[:, None]).sum(-1).amax(dim=2)       # [N, Lq, H]: sum_d |dO v|, the largest over the (equal) keys
    fq = 2.0 ** -20 * scale * a[..., None] * kd.abs().amax(dim=1, keepdim=True)
    fk = 2.0 ** -20 * scale * (a[..., None] * qd.abs()).sum(dim=1, keepdim=True).expand(-1, Lk, -1, -1) / Lk
    return fq, fk


def _check(label, q, k, v, do, scale, zero_qk=False):
    """Both measures of dQ, dK, dV against fp64 <= 2x the yardstick's on the same inputs; zero_qk: dQ and dK are zero in exact
    arithmetic and are held to the floor instead.  Also: the output under grad is the no-grad output, bit for bit."""
    dt = q.dtype
    out, dq, dk, dv = _run(q, k, v, do, scale)
    with torch.no_grad():
        plain = AG.attention(q, k, v, scale)
        if abs(scale - q.shape[3] ** -0.5) < 1e-12:
            assert torch.equal(sdpa(q, k, v), out), f"{label}: the seam's no-grad output differs from the output under grad"
    assert torch.equal(plain, out), f"{label}: forward under grad differs from the no-grad forward"
    ref = R.grads64(q, k, v, do, scale)
    yd = R.yardstick(q, k, v, do, scale, dt)
    fq, fk = _floor(q, k, v, do, scale) if zero_qk else (None, None)
    for name, g, r, y, fl in (("dq", dq, ref[1], yd[1], fq), ("dk", dk, ref[2], yd[2], fk), ("dv", dv, ref[3], yd[3], None)):
        assert g.dtype == dt and g.shape == r.shape and torch.isfinite(g).all(), (label, name)
        if fl is not None:
            worst = float((g.double().abs() / fl.clamp_min(1e-300)).max())
            print(f"{label} {_name(dt)} {name}: exact zero; largest |g| {float(g.abs().max()):.2e} = {worst:.3f} of the floor")
            assert bool((g.double().abs() <= fl).all()), (label, name, worst)
            continue
        e, ey = R.rel_l2(g, r), R.rel_l2(y, r)
        b, by = R.worst_block(g, r), R.worst_block(y, r)
        print(f"{label} {_name(dt)} {name}: rel L2 hip {e:.2e} yardstick {ey:.2e} ({_ratio(e, ey)}); worst block hip {b:.2e} yardstick {by:.2e} ({_ratio(b, by)})")
        assert e <= 2 * ey, (label, name, e, ey)
        assert b <= 2 * by, (label, name, b, by)


@pytest.mark.parametrize("dt", DTYPES, ids=_name)
@pytest.mark.parametrize("shape", list(MODEL_SHAPES), ids=str)
def test_model_shapes_against_fp64(cuda, shape, dt):
    N, Lq, Lk, H, C = MODEL_SHAPES[shape]
    q, k, v, do = R.make_inputs(N, Lq, Lk, H, C, dt, device=cuda, seed=Lq + Lk)
    _check(shape, q, k, v, do, C ** -0.5)


@pytest.mark.parametrize("dt", DTYPES, ids=_name)
@pytest.mark.parametrize("C", [32, 64])
def test_edge_lengths_against_fp64(cuda, C, dt):
    for Lq, Lk in EDGE_PAIRS:
        q, k, v, do = R.make_inputs(2, Lq, Lk, 3, C, dt, device=cuda, seed=1000 * Lq + Lk)
        _check(f"Lq {Lq} Lk {Lk} d {C}", q, k, v, do, C ** -0.5, zero_qk=(Lk == 1))


@pytest.mark.parametrize("dt", DTYPES, ids=_name)
@pytest.mark.parametrize("C", [32, 64])
def test_peaked_softmax_against_fp64(cuda, C, dt):
    for Lq, Lk in [(24, 24), (300, 200), (130, 1370)]:
        q, k, v, do = R.make_inputs(2, Lq, Lk, 4, C, dt, device=cuda, seed=Lq, gain=4.0)
        _check(f"operands x4, Lq {Lq} Lk {Lk} d {C}", q, k, v, do, C ** -0.5)
        q, k, v, do = R.make_inputs(2, Lq, Lk, 4, C, dt, device=cuda, seed=Lq + 1, spike=(5, 30.0))
        _check(f"one large query, Lq {Lq} Lk {Lk} d {C}", q, k, v, do, C ** -0.5)
        q, k, v, do = R.make_inputs(2, Lq, Lk, 4, C, dt, device=cuda, seed=Lq + 2)
        _check(f"softmax_scale 0.35, Lq {Lq} Lk {Lk} d {C}", q, k, v, do, 0.35)


def _bar(label, g, r, y):
    e, ey = R.rel_l2(g, r), R.rel_l2(y, r)
    b, by = R.worst_block(g, r), R.worst_block(y, r)
    print(f"{label}: rel L2 hip {e:.2e} yardstick {ey:.2e}; worst block hip {b:.2e} yardstick {by:.2e}")
    assert e <= 2 * ey and b <= 2 * by, (label, e, ey, b, by)


@pytest.mark.parametrize("dt", DTYPES, ids=_name)
@pytest.mark.parametrize("C", [32, 64])
def test_the_seam_carries_gradients_in_all_three_call_forms(cuda, C, dt):
    N, L, Lk, H = 2, 200, 77, 4
    q, k, v, do = R.make_inputs(N, L, L, H, C, dt, device=cuda, seed=7)
    scale = C ** -0.5
    ref, yd = R.grads64(q, k, v, do, scale), R.yardstick(q, k, v, do, scale, dt)

    # (qkv): before the backward existed this call returned an output detached from qkv
    qkv = torch.stack([q, k, v], dim=2).requires_grad_(True)
    out = sdpa(qkv)
    assert out.requires_grad and out.dtype == dt
    out.backward(do)
    assert qkv.grad is not None and qkv.grad.shape == qkv.shape and qkv.grad.dtype == dt
    for i, name in enumerate(("dq", "dk", "dv")):
        _bar(f"(qkv) d {C} {_name(dt)} {name}", qkv.grad[:, :, i], ref[1 + i], yd[1 + i])
    with torch.no_grad():
        assert torch.equal(sdpa(qkv), out)

    # 3 * loss: three times the gradient, within the same bar (the cotangent 3 dO is another 16-bit tensor)
    qkv3 = qkv.detach().clone().requires_grad_(True)
    (3.0 * (sdpa(qkv3).float() * do.float()).sum()).backward()
    ref3, yd3 = R.grads64(q, k, v, 3 * do, scale), R.yardstick(q, k, v, 3 * do, scale, dt)
    for i, name in enumerate(("dq", "dk", "dv")):
        _bar(f"3 x loss d {C} {_name(dt)} {name}", qkv3.grad[:, :, i], ref3[1 + i], yd3[1 + i])
        _bar(f"3 x loss against 3 x gradient d {C} {_name(dt)} {name}", qkv3.grad[:, :, i], 3 * ref[1 + i], 3 * yd[1 + i].double())

    # (q, kv) with another key length
    q2, k2, v2, do2 = R.make_inputs(N, L, Lk, H, C, dt, device=cuda, seed=8)
    ref2, yd2 = R.grads64(q2, k2, v2, do2, scale), R.yardstick(q2, k2, v2, do2, scale, dt)
    qq = q2.clone().requires_grad_(True)
    kv = torch.stack([k2, v2], dim=2).requires_grad_(True)
    sdpa(qq, kv).backward(do2)
    _bar(f"(q, kv) d {C} {_name(dt)} dq", qq.grad, ref2[1], yd2[1])
    _bar(f"(q, kv) d {C} {_name(dt)} dk", kv.grad[:, :, 0], ref2[2], yd2[2])
    _bar(f"(q, kv) d {C} {_name(dt)} dv", kv.grad[:, :, 1], ref2[3], yd2[3])

    # (q, k, v): strided views cut from one projection output [N, L, 3 H C]
    proj = torch.cat([t.reshape(N, L, H * C) for t in (q, k, v)], dim=-1).requires_grad_(True)
    views = [proj[..., i * H * C:(i + 1) * H * C].reshape(N, L, H, C) for i in range(3)]
    assert not views[1].is_contiguous()
    sdpa(*views).backward(do)
    for i, name in enumerate(("dq", "dk", "dv")):
        _bar(f"(q, k, v) views d {C} {_name(dt)} {name}", proj.grad[..., i * H * C:(i + 1) * H * C].reshape(N, L, H, C), ref[1 + i], yd[1 + i])

    # only v, only q
    for who in (2, 0):
        leaves = [t.clone().requires_grad_(i == who) for i, t in enumerate((q, k, v))]
        sdpa(*leaves).backward(do)
        assert all((t.grad is None) == (i != who) for i, t in enumerate(leaves))
        _bar(f"only {'qkv'[who]} requires grad d {C} {_name(dt)}", leaves[who].grad, ref[1 + who], yd[1 + who])
    with torch.no_grad():                                     # no grad, no graph: the inference path
        assert not sdpa(q.clone().requires_grad_(True), k, v).requires_grad


def test_fp32_inputs_under_autocast_get_fp32_gradients(cuda):
    N, L, H, C = 2, 96, 4, 32
    g = torch.Generator().manual_seed(11)
    qkv32 = torch.randn((N, L, 3, H, C), generator=g).to(cuda).requires_grad_(True)
    do = torch.randn((N, L, H, C), generator=g).to(cuda)
    with torch.autocast("cuda", dtype=torch.float16):
        out = sdpa(qkv32)
    assert out.dtype == torch.float32 and out.requires_grad
    out.backward(do)
    assert qkv32.grad is not None and qkv32.grad.dtype == torch.float32
    q, k, v = (t.to(torch.float16) for t in qkv32.detach().unbind(dim=2))
    do16 = do.to(torch.float16)
    ref, yd = R.grads64(q, k, v, do16, C ** -0.5), R.yardstick(q, k, v, do16, C ** -0.5, torch.float16)
    for i, name in enumerate(("dq", "dk", "dv")):
        _bar(f"autocast fp16 {name}", qkv32.grad[:, :, i], ref[1 + i], yd[1 + i])


@pytest.mark.parametrize("dt", DTYPES, ids=_name)
@pytest.mark.parametrize("shape", ["dit_spatial", "static_cross"])
def test_backward_is_deterministic(cuda, shape, dt):
    N, Lq, Lk, H, C = MODEL_SHAPES[shape]
    q, k, v, do = R.make_inputs(N, Lq, Lk, H, C, dt, device=cuda, seed=3)
    first = _run(q, k, v, do)
    again = _run(q, k, v, do)
    for a, b in zip(first, again):
        assert torch.equal(a, b)
    # the same call while another, different problem runs on a second stream
    q2, k2, v2, do2 = R.make_inputs(3, 700, 333, 8, 64, dt, device=cuda, seed=4)
    with torch.no_grad():
        out, out2 = AG.attention(q, k, v), AG.attention(q2, k2, v2)
    quiet2 = AG.attention_backward(q2, k2, v2, out2, do2, 0.125)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(4):
            busy2 = AG.attention_backward(q2, k2, v2, out2, do2, 0.125)
    busy = AG.attention_backward(q, k, v, out, do, C ** -0.5)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for a, b in zip(first[1:], busy):
        assert torch.equal(a, b)
    for a, b in zip(quiet2, busy2):
        assert torch.equal(a, b)


@pytest.mark.parametrize("dt", DTYPES, ids=_name)
@pytest.mark.parametrize("C", [32, 64])
def test_zero_and_trivial_cases(cuda, C, dt):
    scale = C ** -0.5
    for Lq, Lk in [(24, 24), (130, 200)]:
        q, k, v, do = R.make_inputs(2, Lq, Lk, 3, C, dt, device=cuda, seed=Lq)
        _, dq, dk, dv = _run(q, k, v, torch.zeros_like(do))
        assert not dq.any() and not dk.any() and not dv.any(), "dout = 0 must give exact zeros"
        # all keys (and values) identical: uniform probabilities, dQ = dK = 0 in exact arithmetic, dV = sum_q dO / Lk
        k1, v1 = k[:, :1].expand(-1, Lk, -1, -1).contiguous(), v[:, :1].expand(-1, Lk, -1, -1).contiguous()
        _check(f"identical keys Lq {Lq} Lk {Lk} d {C}", q, k1, v1, do, scale, zero_qk=True)
        dv1 = _run(q, k1, v1, do)[3]
        want = (do.double().sum(dim=1, keepdim=True) / Lk).expand(-1, Lk, -1, -1)
        e, ey = R.rel_l2(dv1, want), R.rel_l2(R.yardstick(q, k1, v1, do, scale, dt)[3], want)
        print(f"identical keys Lq {Lq} Lk {Lk} d {C} {_name(dt)}: dv against sum dO / Lk: hip {e:.2e} yardstick {ey:.2e}")
        assert e <= 2 * ey
    # empty sequences: zeros of the right shapes, no launch
    for Lq, Lk in [(0, 7), (5, 0), (0, 0)]:
        q = torch.randn((2, Lq, 3, C), device=cuda).to(dt).requires_grad_(True)
        k = torch.randn((2, Lk, 3, C), device=cuda).to(dt).requires_grad_(True)
        v = torch.randn((2, Lk, 3, C), device=cuda).to(dt).requires_grad_(True)
        out = AG.attention(q, k, v)
        assert out.shape == (2, Lq, 3, C) and not out.any()
        out.backward(torch.ones_like(out))
        for t in (q, k, v):
            assert t.grad is not None and t.grad.shape == t.shape and not t.grad.any()


# ---- a reference-shaped block: torch fp32 parameters under fp16 autocast around the seam
class _RefFn(torch.autograd.Function):
    """The attention operator with the gradient as tests/attn_bwd_ref.py computes it: which = 0 the float64 formula, 1 the yardstick.
    The forward value is the kernel's in every variant, so the cotangents that reach the attention are identical and the comparison of
    the parameter gradients isolates the backward.  (autocast off inside: the references' fp32 products must stay fp32)"""

    @staticmethod
    def forward(ctx, q, k, v, which):
        ctx.save_for_backward(q, k, v)
        ctx.which = which
        with torch.no_grad():
            return AG.attention(q, k, v)

    @staticmethod
    def backward(ctx, do):
        q, k, v = ctx.saved_tensors
        scale = q.shape[3] ** -0.5
        with torch.autocast("cuda", enabled=False):
            if ctx.which == 0:
                return tuple(t.to(q.dtype) for t in R.grads64(q, k, v, do, scale)[1:]) + (None,)
            return tuple(R.yardstick(q, k, v, do, scale, q.dtype)[1:]) + (None,)


class _Block(nn.Module):
    def __init__(self, dim=128, heads=4, ctx_dim=96):
        super().__init__()
        self.heads, self.hd = heads, dim // heads
        self.n1, self.n2 = nn.LayerNorm(dim), nn.LayerNorm(dim)
        self.qkv, self.proj1 = nn.Linear(dim, 3 * dim), nn.Linear(dim, dim)
        self.qn1, self.kn1 = MultiHeadRMSNorm(self.hd, heads), MultiHeadRMSNorm(self.hd, heads)
        self.to_q, self.to_kv, self.proj2 = nn.Linear(dim, dim), nn.Linear(ctx_dim, 2 * dim), nn.Linear(dim, dim)
        self.qn2, self.kn2 = MultiHeadRMSNorm(self.hd, heads), MultiHeadRMSNorm(self.hd, heads)
        self.attend = None                           # None: the seam; 0 / 1: _RefFn

    def _attn(self, q, k, v):
        if self.attend is None:
            return sdpa(q, k, v)
        lp = torch.float16
        return _RefFn.apply(q.to(lp), k.to(lp), v.to(lp), self.attend).to(q.dtype)

    def forward(self, x, ctx):
        N, L, _ = x.shape
        q, k, v = self.qkv(self.n1(x)).reshape(N, L, 3, self.heads, self.hd).unbind(dim=2)
        x = x + self.proj1(self._attn(self.qn1(q), self.kn1(k), v).reshape(N, L, -1))
        q = self.to_q(self.n2(x)).reshape(N, L, self.heads, self.hd)
        k, v = self.to_kv(ctx).reshape(N, ctx.shape[1], 2, self.heads, self.hd).unbind(dim=2)
        return x + self.proj2(self._attn(self.qn2(q), self.kn2(k), v).reshape(N, L, -1))


def test_a_reference_shaped_block_trains(cuda):
    torch.manual_seed(0)
    block = _Block().to(cuda)
    g = torch.Generator().manual_seed(1)
    x, ctx = torch.randn((2, 80, 128), generator=g).to(cuda), torch.randn((2, 50, 96), generator=g).to(cuda)
    target = torch.randn((2, 80, 128), generator=g).to(cuda)
    params = [p for p in block.parameters()]

    def loss_fn():
        with torch.autocast("cuda", dtype=torch.float16):
            y = block(x, ctx)
        return ((y.float() - target) ** 2).sum(dim=-1).mean()

    grads = {}
    for which in (0, 1, None):
        block.attend = which
        block.zero_grad(set_to_none=True)
        loss_fn().backward()
        grads[which] = [p.grad.detach().clone() for p in params]
    for (name, _), g64, gy, gh in zip(block.named_parameters(), grads[0], grads[1], grads[None]):
        e, ey = R.rel_l2(gh, g64), R.rel_l2(gy, g64)
        print(f"block {name}: grad rel L2 from the fp64-attention block: hip {e:.2e} yardstick {ey:.2e}")
        assert torch.isfinite(gh).all() and gh.dtype == torch.float32
        assert e <= 2 * ey, (name, e, ey)

    block.attend = None
    opt = torch.optim.AdamW(params, lr=2e-3)
    losses = [training.train_step(params, opt, loss_fn)["loss"] for _ in range(30)]
    print(f"block training: loss {losses[0]:.4f} -> {losses[-1]:.4f} after 30 AdamW steps (ratio {losses[-1] / losses[0]:.3f})")
    assert all(l == l for l in losses) and losses[-1] < losses[0]
