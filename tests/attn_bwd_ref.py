"""References for the attention backward (csrc/attn_bwd.hip), plain torch, any device.

grads64    the float64 O, dQ, dK, dV of softmax(q k^T * scale) v from the 16-bit operands, written out by formula.
yardstick  the same computation as an fp32 composition with the kernel's rounding points (flash-attn's contract): scores and dP in
           fp32 from the 16-bit operands, P rounded to the operand type where it feeds dV, dS = P (dP - delta) scale rounded where it
           feeds dQ and dK, delta from the ROUNDED O, gradients rounded to the operand type.  Its distance from grads64 is the unit in
           which every GPU bar is expressed.
rel_l2 / worst_block  the two error measures.

Tensors are [N, L, H, C]; q, dO have Lq rows, k, v have Lk rows."""
import torch


def _heads_first(t, dtype):
    return t.to(dtype).permute(0, 2, 1, 3)          # [N, H, L, C]


def grads64(q16, k16, v16, do16, scale):
    q, k, v, do = (_heads_first(t, torch.float64) for t in (q16, k16, v16, do16))
    s = torch.matmul(q, k.transpose(-1, -2)) * float(scale)                 # [N, H, Lq, Lk]
    s = s - s.amax(dim=-1, keepdim=True)
    p = torch.exp(s)
    p = p / p.sum(dim=-1, keepdim=True)
    o = torch.matmul(p, v)
    dv = torch.matmul(p.transpose(-1, -2), do)
    dp = torch.matmul(do, v.transpose(-1, -2))
    delta = (do * o).sum(dim=-1, keepdim=True)
    ds = p * (dp - delta) * float(scale)
    dq = torch.matmul(ds, k)
    dk = torch.matmul(ds.transpose(-1, -2), q)
    return tuple(t.permute(0, 2, 1, 3).contiguous() for t in (o, dq, dk, dv))


def yardstick(q16, k16, v16, do16, scale, dt):
    """(O, dQ, dK, dV) in dtype dt from the fp32 composition with the kernel's rounding points."""
    q, k, v, do = (_heads_first(t, torch.float32) for t in (q16, k16, v16, do16))
    s = torch.matmul(q, k.transpose(-1, -2)) * float(scale)
    lse = torch.logsumexp(s, dim=-1, keepdim=True)
    p = torch.exp(s - lse)                                                   # fp32
    o = torch.matmul(p, v).to(dt)                                            # the forward's rounded output
    p16 = p.to(dt).float()
    dv = torch.matmul(p16.transpose(-1, -2), do).to(dt)
    dp = torch.matmul(do, v.transpose(-1, -2))
    delta = (do * o.float()).sum(dim=-1, keepdim=True)
    ds16 = (p * (dp - delta) * float(scale)).to(dt).float()
    dq = torch.matmul(ds16, k).to(dt)
    dk = torch.matmul(ds16.transpose(-1, -2), q).to(dt)
    return tuple(t.permute(0, 2, 1, 3).contiguous() for t in (o, dq, dk, dv))


def rel_l2(x, ref):
    """||x - ref|| / ||ref|| over the whole tensor (0 / 0 = 0)."""
    x, ref = x.double(), ref.double()
    den = ref.norm().item()
    num = (x - ref).norm().item()
    return 0.0 if num == 0.0 else (num / den if den > 0 else float("inf"))


def worst_block(x, ref, block=32):
    """max over the (sequence, head) problems and the 32-row blocks of a gradient [N, L, H, C] of
    ||err_block|| / (sqrt(rows_block / L) * ||ref_problem||): a dropped, doubled or misplaced tile of one head shows here, where the
    whole-tensor figure averages it away."""
    x, ref = x.double(), ref.double()
    N, L, H, C = ref.shape
    err2 = ((x - ref) ** 2).sum(dim=-1)                                      # [N, L, H]
    nb = (L + block - 1) // block
    pad = nb * block - L
    if pad:
        err2 = torch.cat([err2, err2.new_zeros((N, pad, H))], dim=1)
    blk = err2.reshape(N, nb, block, H).sum(dim=2).sqrt()                    # [N, nb, H]
    rows = torch.full((nb,), float(block), dtype=torch.float64, device=ref.device)
    if pad:
        rows[-1] = block - pad
    ref_norm = (ref ** 2).sum(dim=(1, 3)).sqrt()                             # [N, H]
    den = (rows / L).sqrt()[None, :, None] * ref_norm[:, None, :]
    ratio = torch.where(blk == 0, torch.zeros_like(blk), blk / den)
    return float(ratio.max().item())


def make_inputs(N, Lq, Lk, H, C, dt, device="cpu", seed=0, gain=1.0, spike=None):
    """Standard-normal q, k, v, dO in dtype dt (operands times `gain`); spike = (query index, factor) enlarges one query of every
    problem, which concentrates its softmax on one key."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    q = torch.randn((N, Lq, H, C), generator=g) * gain
    k = torch.randn((N, Lk, H, C), generator=g) * gain
    v = torch.randn((N, Lk, H, C), generator=g) * gain
    do = torch.randn((N, Lq, H, C), generator=g)
    if spike is not None:
        q[:, spike[0] % Lq] *= spike[1]
    return tuple(t.to(device=device, dtype=dt) for t in (q, k, v, do))
