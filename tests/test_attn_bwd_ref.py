"""The references of the attention backward (tests/attn_bwd_ref.py) on the host: the float64 formula against torch double autograd and
central finite differences, and the yardstick's distance from it pinned to the range the number formats give -- a broken yardstick
cannot loosen the GPU bars unnoticed."""
import pytest
import torch

import attn_bwd_ref as R

# (problems, Lq, Lk, head_dim): the shapes the GPU bars were sized on
SHAPES = [(4, 512, 512, 32), (4, 24, 24, 32), (2, 512, 1370, 32), (2, 300, 4096, 32), (2, 1000, 512, 64), (4, 77, 130, 64)]


def _autograd64(q16, k16, v16, do16, scale):
    q, k, v = (t.double().requires_grad_(True) for t in (q16, k16, v16))
    s = torch.einsum("nqhc,nkhc->nhqk", q, k) * scale
    o = torch.einsum("nhqk,nkhc->nqhc", torch.softmax(s, dim=-1), v)
    o.backward(do16.double())
    return o.detach(), q.grad, k.grad, v.grad


@pytest.mark.parametrize("shape", [(2, 37, 53, 3, 32), (1, 24, 24, 2, 64), (2, 1, 9, 1, 32), (1, 70, 1, 2, 64)])
@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
def test_formula_matches_double_autograd(shape, dt):
    N, Lq, Lk, H, C = shape
    q, k, v, do = R.make_inputs(N, Lq, Lk, H, C, dt, seed=Lq + Lk)
    scale = 0.7 * C ** -0.5
    for name, mine, ref in zip(("o", "dq", "dk", "dv"), R.grads64(q, k, v, do, scale), _autograd64(q, k, v, do, scale)):
        assert mine.shape == ref.shape and mine.dtype == torch.float64
        err = (mine - ref).norm().item()
        assert err <= 1e-12 * max(ref.norm().item(), 1e-300) + 1e-300 or err <= 1e-12 * ref.norm().item(), (name, err)


def test_formula_matches_central_differences():
    N, Lq, Lk, H, C = 1, 3, 4, 1, 32
    q, k, v, do = R.make_inputs(N, Lq, Lk, H, C, torch.float16, seed=5)
    scale = C ** -0.5
    _, dq, dk, dv = R.grads64(q, k, v, do, scale)

    def loss(q_, k_, v_):
        s = torch.einsum("nqhc,nkhc->nhqk", q_, k_) * scale
        return (torch.einsum("nhqk,nkhc->nqhc", torch.softmax(s, dim=-1), v_) * do.double()).sum().item()

    base = [t.double() for t in (q, k, v)]
    h = 1e-5
    for which, g in enumerate((dq, dk, dv)):
        for idx in [(0, 0, 0, 0), (0, 1, 0, 7), (0, 2, 0, 31)]:
            plus, minus = [t.clone() for t in base], [t.clone() for t in base]
            plus[which][idx] += h
            minus[which][idx] -= h
            fd = (loss(*plus) - loss(*minus)) / (2 * h)
            assert abs(fd - g[idx].item()) <= 1e-7 * max(1.0, abs(fd)), (which, idx, fd, g[idx].item())


# Whole-tensor relative L2 of the yardstick from fp64, as measured on the host when the GPU bars were sized: 2.3-2.5e-3 (bf16) and
# 2.9-3.2e-4 (fp16) with standard-normal operands on the six shapes above, rising to 6-8e-3 (bf16) and about 1e-3 (fp16) for dQ / dK
# when the operands are scaled by 4 (head_dim 32) or 3 (head_dim 64) and the softmax is peaked.  That is three (peaked: up to ten)
# single roundings of the format -- 2^-(p+1) / sqrt(3) * 0.72 rms over a binade, 8.1e-4 for bf16 (p = 8), 1.0e-4 for fp16 (p = 11):
# P or dS, the rounded O inside delta, and the stored result.  The pins are those ranges with a quarter of slack either way; half on the peaked figures, which were given
# to one digit and scatter more (a 24 x 24 problem with a peaked softmax is a sample of few terms).
PIN = {torch.bfloat16: (2.3e-3 * 0.75, 2.5e-3 * 1.25, 8e-3 * 1.5), torch.float16: (2.9e-4 * 0.75, 3.2e-4 * 1.25, 1e-3 * 1.5)}


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
def test_yardstick_distance_is_what_the_formats_give(shape, dt):
    P, Lq, Lk, C = shape
    lo, hi, hi_peaked = PIN[dt]
    for gain, top in ((1.0, hi), (4.0 if C == 32 else 3.0, hi_peaked)):
        q, k, v, do = R.make_inputs(P // 2, Lq, Lk, 2, C, dt, seed=P + Lq + Lk + C, gain=gain)
        scale = C ** -0.5
        ref = R.grads64(q, k, v, do, scale)
        yd = R.yardstick(q, k, v, do, scale, dt)
        for name, y, r in zip(("o", "dq", "dk", "dv"), yd, ref):
            assert y.dtype == dt and y.shape == r.shape
            e, wb = R.rel_l2(y, r), R.worst_block(y, r)
            print(f"{shape} {str(dt)[6:]} gain {gain}: {name} rel L2 {e:.2e} worst block {wb:.2e} ({wb / e:.2f}x)")
            if name == "o":
                continue
            assert lo <= e <= top, (name, e)
            assert 0.9 * e <= wb <= 4 * e, (name, e, wb)     # measured 1.0-2.6x: a block is a sample of the same error


def test_worst_block_sees_a_dropped_tile():
    """One 32-row block of one head zeroed: the whole-tensor figure of a large batch barely moves, the worst block is ~1."""
    g = torch.Generator().manual_seed(3)
    ref = torch.randn((8, 256, 8, 32), generator=g, dtype=torch.float64)
    x = ref.clone()
    x[5, 64:96, 3] = 0
    assert R.rel_l2(x, ref) < 0.05
    assert 0.8 < R.worst_block(x, ref) < 1.25
    assert R.worst_block(ref, ref) == 0.0 and R.rel_l2(ref, ref) == 0.0
    short = ref[:, :40]                                       # a last block of 8 rows is weighed by its share of the rows
    y = short.clone()
    y[0, 32:40, 0] = 0
    assert 0.7 < R.worst_block(y, short) < 1.4
