"""References for the ragged attention backward (gvf_attn_varlen_bwd): tests/attn_bwd_ref.py looped over the sequences of a packed batch.

Tensors are packed [T, H, C]: q, dO follow q_lens, k, v follow k_lens.  A sequence without keys has zero output rows and zero dQ (the
forward's contract); one without queries has zero dK and dV.

packed_grads64 / packed_yardstick   (O, dQ, dK, dV) packed, from grads64 / yardstick of every non-empty sequence.
block_diagonal_grads64              the same four from ONE dense masked float64 computation differentiated by autograd: the independent
                                    check of the loop (tests/test_attn_varlen_bwd_host.py).
bounds / cu / make_packed           the slices, the cu_seqlens tensor and seeded operands by make_inputs' recipe."""
import torch

import attn_bwd_ref as R


def bounds(lens):
    out, at = [], 0
    for n in lens:
        out.append((at, at + n))
        at += n
    return out


def cu(lens, device="cpu"):
    return torch.tensor([0] + [b for _, b in bounds(lens)], dtype=torch.int32, device=device)


def make_packed(q_lens, k_lens, H, C, dt, device="cpu", seed=0):
    """Standard-normal packed q, k, v, dO in dtype dt (make_inputs with one batch element of the total lengths)."""
    q, k, v, do = R.make_inputs(1, max(1, sum(q_lens)), max(1, sum(k_lens)), H, C, dt, device=device, seed=seed)
    return q[0, :sum(q_lens)], k[0, :sum(k_lens)], v[0, :sum(k_lens)], do[0, :sum(q_lens)]


def _looped(fn, q, k, v, do, q_lens, k_lens, out_dtype):
    o, dq = (torch.zeros(q.shape, dtype=out_dtype, device=q.device) for _ in range(2))
    dk, dv = (torch.zeros(k.shape, dtype=out_dtype, device=k.device) for _ in range(2))
    for (a, b), (c, d) in zip(bounds(q_lens), bounds(k_lens)):
        if b > a and d > c:
            so, sq, sk, sv = fn(q[None, a:b], k[None, c:d], v[None, c:d], do[None, a:b])
            o[a:b], dq[a:b], dk[c:d], dv[c:d] = so[0], sq[0], sk[0], sv[0]
    return o, dq, dk, dv


def packed_grads64(q, k, v, do, q_lens, k_lens, scale):
    return _looped(lambda *t: R.grads64(*t, scale), q, k, v, do, q_lens, k_lens, torch.float64)


def packed_yardstick(q, k, v, do, q_lens, k_lens, scale, dt):
    return _looped(lambda *t: R.yardstick(*t, scale, dt), q, k, v, do, q_lens, k_lens, dt)


def block_diagonal_grads64(q, k, v, do, q_lens, k_lens, scale):
    q, k, v = (t.double().detach().clone().requires_grad_(True) for t in (q, k, v))
    mask = torch.zeros((q.shape[0], k.shape[0]), dtype=torch.bool, device=q.device)
    for (a, b), (c, d) in zip(bounds(q_lens), bounds(k_lens)):
        mask[a:b, c:d] = True
    s = torch.einsum("qhc,khc->hqk", q, k) * float(scale)
    s = torch.where(mask[None], s, torch.full_like(s, -1e300))
    e = torch.exp(s - s.amax(dim=-1, keepdim=True)) * mask[None]             # a row without keys: all zeros
    p = e / e.sum(dim=-1, keepdim=True).clamp_min(1e-300)
    o = torch.einsum("hqk,khc->qhc", p, v)
    o.backward(do.double())
    return o.detach(), q.grad, k.grad, v.grad


def per_sequence(x, ref, lens):
    """[(sequence index, x rows, ref rows)] as [1, L, H, C] tensors for the measures of attn_bwd_ref, non-empty sequences only."""
    return [(i, x[None, a:b], ref[None, a:b]) for i, (a, b) in enumerate(bounds(lens)) if b > a]
