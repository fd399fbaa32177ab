"""Element-wise conformance of gvf_attn_fwd / gvf_attn_varlen_fwd (csrc/attn.hip) -- the one-wave short-sequence kernel, the K/V-resident
kernel and the streaming kernel behind one router -- against the float64 reference of tests/attn_ref.py.  Every case checks (a) every output
element within attn_ref's bound of the path the router takes, (b) nothing outside the output view written (a view with o_sl > H * D and
rows after Lq inside a buffer pre-filled with a 16-bit sentinel), (c) no read of q / k / v outside the problem (views whose padding channels
and rows past each key set hold NaN; the transposed V's padding keys, which the contract requires finite, hold 1000), (d) the same bits on
a second launch, and prints the worst |err| / bound.  The case matrix is pairwise over the dispatch axes (path, head dim 32 / 64, row-major
/ transposed V, bf16 / fp16, gains none / q / k / both, scale default / 1 / 0.05), the tile edges of Lk and Lq, the strided forms the DiT
uses (K/V shared by all `inner`, the temporal (B,T,N,.) <-> (B,N,T,.) view, q / k / v slices of one packed qkv projection) and varlen
batches (cross form, empty query or key ranges, all sequences empty).

Invariance: a problem's bits do not depend on n_outer / n_inner (the DiT's batch: the per-sample bits of its attention layouts at B = 3 equal
those at B = 1) nor on the q-block its rows fall in.  GVF_ATTN_KVRES is read once per process: test_kvres_modes_in_child_processes re-runs
this file with it at 0 (no K/V-resident kernel) and 2 (wherever it applies, varlen included)."""
import os
import subprocess
import sys

import pytest
import torch

import attn_ref as A
from gvfdiffusion_amd.ops import dit_ops

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.environ.get("GVF_ATTN_CONFORMANCE_CHILD") == "1"
KVRES_MODE = int(os.environ.get("GVF_ATTN_KVRES", "1"))
SENTINEL16 = 0x7E5A                  # a 16-bit pattern no kernel writes here (fp16: a NaN payload; bf16: 7.2e37)
VT_PAD = 1000.0                      # transposed V's padding keys: finite by contract (P = 0 there), large so that a leak shows
WORST = {}


def _path(D, vt, varlen, Lq, Lk):
    """The kernel launch_attn picks (csrc/attn.hip); varlen: Lq / Lk are max_Lq / max(max_Lk, 1)."""
    if D == 32 and not vt and not varlen and Lq <= 32 and Lk <= 32:
        return "small"
    if KVRES_MODE != 0 and Lk <= 512 and Lq >= 128 and (KVRES_MODE == 2 or (D == 64 and vt and Lq >= 1024)):
        return "kvres"
    return "stream"


def _bits(t):
    return t.view(torch.int16) if t.element_size() == 2 else t.view(torch.int32)


def _idx(base, st, O, I, L, H, C):
    """Flat element indices (O, I, L, H, C) of a strided view: base + o s0 + i s1 + l s2 + h s3 + c s4 (s4 = 1 unless given)."""
    ar = [torch.arange(n, dtype=torch.int64) for n in (O, I, L, H, C)]
    sc = st[4] if len(st) > 4 else 1
    return (base + ar[0].view(-1, 1, 1, 1, 1) * st[0] + ar[1].view(1, -1, 1, 1, 1) * st[1] + ar[2].view(1, 1, -1, 1, 1) * st[2]
            + ar[3].view(1, 1, 1, -1, 1) * st[3] + ar[4].view(1, 1, 1, 1, -1) * sc)


def _check(out_h, ref, bnd, what, path):
    """Asserts the bound.  The printed worst |err| / bound is 1.0 whenever an element's error interval lies inside one rounding step (the
    bound is then the distance to the correctly rounded value itself); `wide` is the fraction of elements whose interval spans two or more
    16-bit values -- how much room the fp32-level terms leave."""
    n_bad, worst = A.excess(out_h, ref, bnd)
    wide = float((bnd > (A.r16(ref, out_h.dtype) - ref).abs() * (1 + 1e-12) + 1e-300).double().mean()) if out_h.element_size() == 2 else 1.0
    print(f"{what} [{path}]: max |err| / bound {worst:.3f}, intervals wider than one rounding step {wide:.2e}")
    WORST[path] = max(WORST.get(path, 0.0), worst)
    assert n_bad == 0, f"{what} [{path}]: {n_bad} of {ref.numel()} elements outside the bound (worst {worst:.2f} x)"


def _launch_checked(obuf, out_idx, launch, what):
    """Run `launch` on obuf (sentinel-filled), check that only out_idx was written, relaunch and compare the bits; returns the output elements."""
    before = obuf.clone()
    launch()
    torch.cuda.synchronize()
    after = obuf.clone()
    mask = torch.ones(obuf.numel(), dtype=torch.bool, device=obuf.device)
    mask[out_idx.reshape(-1).to(obuf.device)] = False
    assert torch.equal(_bits(after)[mask], _bits(before)[mask]), f"{what}: a store outside the output view"
    obuf.copy_(before)
    launch()
    torch.cuda.synchronize()
    assert torch.equal(_bits(obuf), _bits(after)), f"{what}: a second launch gave other bits"
    return after[out_idx.to(obuf.device)].cpu()


def _gains(g, H, D, which, side):
    return (1.0 + 0.3 * torch.randn((H, D), generator=g)) if which in (side, "both") else None


def _dense(dt, D, vt, gains, scale, layout, n_outer, n_inner, H, Lq, Lk, seed, dev):
    """Host operands (n_outer, n_inner, L, H, D) and device views in `layout`; returns a dict for _run_dense."""
    g = torch.Generator().manual_seed(seed)
    nk_inner = 1 if layout == "shared" else n_inner
    qh = torch.randn((n_outer, n_inner, Lq, H, D), generator=g).to(dt)
    kh = torch.randn((n_outer, nk_inner, Lk, H, D), generator=g).to(dt)
    vh = torch.randn((n_outer, nk_inner, Lk, H, D), generator=g).to(dt)
    gq, gk = _gains(g, H, D, gains, "q"), _gains(g, H, D, gains, "k")
    P = 8                                                          # padding channels (NaN)
    if layout == "qkv":                                            # one packed (outer*inner, L, 3, H, D + P) projection, self attention
        assert Lq == Lk
        kh, vh = (torch.randn((n_outer, n_inner, Lk, H, D), generator=g).to(dt) for _ in range(2))
        row = 3 * H * (D + P)
        st = (n_inner * (Lq + 1) * row, (Lq + 1) * row, row, D + P)
        bases = (0, H * (D + P), 2 * H * (D + P))
        n = n_outer * n_inner * (Lq + 1) * row
        q_st = k_st = v_st = st
    elif layout == "temporal":                                     # (B, T, N, H, D + P) storage, attention over T: outer B, inner N
        row = H * (D + P)
        q_st = (Lq * n_inner * row, row, n_inner * row, D + P)
        k_st = v_st = (Lk * n_inner * row, row, n_inner * row, D + P)
        bases = (0, 0, 0)
        n = None
    else:                                                          # plain / shared: (outer, inner, L + 2, H, D + P)
        row = H * (D + P)
        q_st = (n_inner * (Lq + 2) * row, (Lq + 2) * row, row, D + P)
        k_st = v_st = (nk_inner * (Lk + 2) * row, 0 if layout == "shared" else (Lk + 2) * row, row, D + P)
        bases = (0, 0, 0)
        n = None

    def buf(size, fill=float("nan")):
        return torch.full((size,), fill, dtype=dt)

    if layout == "qkv":
        one = buf(n)
        one[_idx(0, q_st, n_outer, n_inner, Lq, H, D)] = qh
        one[_idx(bases[1], k_st, n_outer, n_inner, Lk, H, D)] = kh
        one[_idx(bases[2], v_st, n_outer, n_inner, Lk, H, D)] = vh
        d = one.to(dev)
        qd, kd, vd = d, d[bases[1]:], d[bases[2]:]
    else:
        nq = n_outer * n_inner * (Lq + 2) * row
        nk = n_outer * nk_inner * (Lk + 2) * row
        qb, kb = buf(nq), buf(nk)
        qb[_idx(0, q_st, n_outer, n_inner, Lq, H, D)] = qh
        kb[_idx(0, k_st, n_outer, nk_inner, Lk, H, D)] = kh
        if vt:                                                     # [outer][inner][head][d][key], keys padded to 64 (finite), NaN beyond
            Lp = (Lk + 63) // 64 * 64
            ld = Lp + 8
            v_st = (nk_inner * H * D * ld, 0 if layout == "shared" else H * D * ld, ld, D * ld)
            vb = buf(n_outer * nk_inner * H * D * ld)
            vb[_idx(0, (v_st[0], v_st[1], 1, v_st[3], ld), n_outer, nk_inner, Lp, H, D)] = VT_PAD
            vb[_idx(0, (v_st[0], v_st[1], 1, v_st[3], ld), n_outer, nk_inner, Lk, H, D)] = vh
        else:
            vb = buf(nk)
            vb[_idx(0, v_st, n_outer, nk_inner, Lk, H, D)] = vh
        qd, kd, vd = qb.to(dev), kb.to(dev), vb.to(dev)
    if layout == "shared":
        kh, vh = kh.expand(n_outer, n_inner, Lk, H, D), vh.expand(n_outer, n_inner, Lk, H, D)
    o_row = H * D + 8
    o_st = (n_inner * (Lq + 3) * o_row, (Lq + 3) * o_row, o_row, D)
    obuf = torch.full((n_outer * n_inner * (Lq + 3) * o_row,), SENTINEL16, dtype=torch.int16).view(dt).to(dev)
    return dict(qh=qh, kh=kh, vh=vh, gq=gq, gk=gk, qd=qd, kd=kd, vd=vd, obuf=obuf, st=(q_st, k_st, v_st, o_st), dev=dev)


def _problems(x, gq, gk):
    """(outer, inner, L, H, D) -> (outer * inner * H, L, D) problems; gains (H, D) -> (P, D)."""
    O, I, L, H, D = x.shape
    p = x.permute(0, 1, 3, 2, 4).reshape(O * I * H, L, D)
    rep = lambda g: None if g is None else g[None].expand(O * I, H, D).reshape(O * I * H, D)
    return p, rep(gq), rep(gk)


def _run_dense(c, dt, D, vt, scale, n_outer, n_inner, H, Lq, Lk):
    q_st, k_st, v_st, o_st = c["st"]
    dev = c["dev"]
    gqd = None if c["gq"] is None else c["gq"].to(dev)
    gkd = None if c["gk"] is None else c["gk"].to(dev)
    out_view = c["obuf"]

    def launch():
        dit_ops.attention(c["qd"], c["kd"], c["vd"], out_view, n_outer, n_inner, Lq, Lk, H, q_st, k_st, v_st, o_st,
                          gqd, gkd, scale=scale, v_transposed=vt, head_dim=D)
    return launch, _idx(0, o_st, n_outer, n_inner, Lq, H, D)


# (dtype, D, v_transposed, gains, scale, layout, n_outer, n_inner, H, Lq, Lk)
BF, HF = torch.bfloat16, torch.float16
CASES = [
    (BF, 32, False, "none", None, "plain", 2, 1, 2, 1, 1),
    (HF, 32, False, "q", 1.0, "plain", 3, 2, 2, 32, 31),
    (BF, 32, False, "both", 0.05, "temporal", 2, 5, 2, 24, 24),
    (HF, 32, False, "k", None, "plain", 2, 1, 2, 33, 32),
    (BF, 64, True, "both", None, "plain", 1, 1, 2, 1024, 512),
    (HF, 64, True, "none", 1.0, "plain", 1, 1, 1, 2049, 511),
    (BF, 32, False, "both", None, "qkv", 1, 2, 3, 512, 512),
    (HF, 64, False, "q", 0.05, "plain", 2, 1, 2, 129, 513),
    (BF, 32, True, "k", 1.0, "shared", 2, 3, 2, 127, 1370),
    (HF, 32, True, "both", None, "shared", 1, 2, 1, 128, 4097),
    (BF, 64, False, "none", 0.05, "plain", 2, 1, 1, 1, 4097),
    (HF, 32, False, "both", None, "temporal", 2, 3, 2, 63, 63),
    (BF, 64, False, "k", None, "plain", 1, 1, 2, 2049, 65),
    (HF, 64, True, "q", None, "plain", 1, 1, 2, 1024, 64),
    (BF, 32, False, "q", None, "qkv", 2, 1, 2, 33, 33),
    (HF, 32, False, "none", 0.05, "shared", 1, 3, 2, 32, 63),
    (BF, 64, True, "none", None, "plain", 1, 1, 1, 1024, 513),
    (HF, 32, False, "both", 1.0, "plain", 1, 2, 2, 128, 1),
    (BF, 32, True, "q", None, "shared", 1, 2, 2, 1024, 33),
]


@pytest.mark.parametrize("dt,D,vt,gains,scale,layout,n_outer,n_inner,H,Lq,Lk", CASES)
def test_dense_attention_elementwise(cuda, dt, D, vt, gains, scale, layout, n_outer, n_inner, H, Lq, Lk):
    c = _dense(dt, D, vt, gains, scale, layout, n_outer, n_inner, H, Lq, Lk, Lq * 31 + Lk * 7 + D, cuda)
    launch, oidx = _run_dense(c, dt, D, vt, scale, n_outer, n_inner, H, Lq, Lk)
    what = f"{str(dt)[6:]} D{D} {'VT' if vt else 'RM'} gains={gains} scale={scale} {layout} {n_outer}x{n_inner}x{H} Lq{Lq} Lk{Lk}"
    out = _launch_checked(c["obuf"], oidx, launch, what)
    q, gq, gk = _problems(c["qh"], c["gq"], c["gk"])
    k, v = _problems(c["kh"], None, None)[0], _problems(c["vh"], None, None)[0]
    path = _path(D, vt, False, Lq, Lk)
    ref, bnd = A.model(q, k, v, path, scale=scale, gq=gq, gk=gk)
    _check(_problems(out, None, None)[0], ref, bnd, what, path)


def _packed(lens, H, D, dt, g, pad_rows):
    """A packed (sum(lens) + pad_rows, H, D + 8) buffer, NaN in its padding, and the host rows."""
    T = sum(lens)
    x = torch.randn((T, H, D), generator=g).to(dt)
    b = torch.full((T + pad_rows, H, D + 8), float("nan"), dtype=dt)
    b[:T, :, :D] = x
    return x, b


# (dtype, D, gains, scale, q_lens, k_lens): self (q_lens == k_lens) and cross; sequences with no queries, no keys, and all empty
VARLEN = [
    (BF, 32, "both", None, [1, 129, 0, 33, 64], [1, 129, 0, 33, 64]),
    (HF, 64, "q", 1.0, [127, 0, 2049, 65, 5, 7], [513, 40, 1, 0, 64, 0]),
    (BF, 64, "none", 0.05, [128, 300, 1, 9], [512, 33, 0, 511]),
    (HF, 32, "k", None, [1024, 31, 0], [4097, 63, 5]),
    (BF, 32, "none", None, [5, 130], [0, 0]),
    (HF, 64, "both", None, [0, 0], [0, 0]),
]


@pytest.mark.parametrize("dt,D,gains,scale,q_lens,k_lens", VARLEN)
def test_varlen_attention_elementwise(cuda, dt, D, gains, scale, q_lens, k_lens):
    g = torch.Generator().manual_seed(sum(q_lens) + 3 * sum(k_lens) + D)
    H = 2
    qh, qb = _packed(q_lens, H, D, dt, g, 2)
    kh, kb = _packed(k_lens, H, D, dt, g, 3)
    vh, vb = _packed(k_lens, H, D, dt, g, 3)
    gq, gk = _gains(g, H, D, gains, "q"), _gains(g, H, D, gains, "k")
    cu = lambda lens: torch.tensor([0] + list(torch.tensor(lens).cumsum(0).tolist()), dtype=torch.int32, device=cuda)
    Tq = sum(q_lens)
    o_row = H * D + 8
    r0 = 2             # two launches write interleaved rows (o_sl = 2 rows): the first from row 2, the second from row 3; 3 rows follow
    obuf = torch.full(((2 * Tq + r0 + 3) * o_row,), SENTINEL16, dtype=torch.int16).view(dt).to(cuda)
    qd, kd, vd = qb.to(cuda), kb.to(cuda), vb.to(cuda)
    gqd = None if gq is None else gq.to(cuda)
    gkd = None if gk is None else gk.to(cuda)
    cq, ck = cu(q_lens), cu(k_lens)
    row = H * (D + 8)

    def launcher(r):
        return lambda: dit_ops.attention_varlen(qd, kd, vd, obuf[r * o_row:], cq, ck, max(q_lens), max(k_lens), H, (0, 0, row, D + 8),
                                                (0, 0, row, D + 8), (0, 0, row, D + 8), (0, 0, 2 * o_row, D), gqd, gkd, scale=scale, head_dim=D)
    what = f"varlen {str(dt)[6:]} D{D} gains={gains} scale={scale} q{q_lens} k{k_lens}"
    out = _launch_checked(obuf, _idx(r0 * o_row, (0, 0, 2 * o_row, D), 1, 1, Tq, H, D), launcher(r0), what)[0, 0]     # (Tq, H, D)
    out2 = _launch_checked(obuf, _idx((r0 + 1) * o_row, (0, 0, 2 * o_row, D), 1, 1, Tq, H, D), launcher(r0 + 1), what + " (2nd region)")
    assert torch.equal(_bits(out2[0, 0]), _bits(out)), f"{what}: the interleaved launch gave other bits"
    path = _path(D, False, True, max(q_lens), max(max(k_lens), 1))
    q0 = k0 = 0
    for Lq, Lk in zip(q_lens, k_lens):
        o = out[q0:q0 + Lq]
        if Lq and not Lk:
            assert bool((_bits(o) == 0).all()), f"{what}: a sequence without keys must give zero rows"
        elif Lq:
            ref, bnd = A.model(qh[q0:q0 + Lq].permute(1, 0, 2), kh[k0:k0 + Lk].permute(1, 0, 2), vh[k0:k0 + Lk].permute(1, 0, 2), path,
                               scale=scale, gq=gq, gk=gk)
            _check(o.permute(1, 0, 2), ref, bnd, f"{what} seq Lq{Lq} Lk{Lk}", path)
        q0, k0 = q0 + Lq, k0 + Lk


def test_empty_key_range_through_the_sparse_seam(cuda):
    """sparse_scaled_dot_product_attention with a sparse kv whose middle batch element is empty: that element's queries get zeros (as
    flash-attn's varlen kernel writes), the others what they get alone."""
    from gvfdiffusion_amd.sparse import SparseTensor
    from gvfdiffusion_amd.sparse.attention import sparse_scaled_dot_product_attention as spa
    g = torch.Generator().manual_seed(5)
    H, C = 2, 32
    coords = torch.zeros((70, 4), dtype=torch.int32)
    coords[40:, 0] = 2                                             # batch 0: 40 keys, batch 1: none, batch 2: 30
    kv = SparseTensor(torch.randn((70, 2, H, C), generator=g).to(torch.bfloat16).to(cuda), coords.to(cuda))
    q = torch.randn((3, 33, H, C), generator=g).to(torch.bfloat16).to(cuda)
    out = spa(q, kv)
    assert kv.layout[1].stop == kv.layout[1].start and bool((_bits(out[1]) == 0).all())
    alone = SparseTensor(kv.feats[40:], torch.zeros((30, 4), dtype=torch.int32, device=cuda))
    assert torch.equal(out[2], spa(q[2:], alone)[0])


# ---- invariance ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt,D,vt,layout,Lq,Lk", [(BF, 32, False, "plain", 24, 24), (HF, 32, False, "temporal", 24, 24),
                                                 (BF, 32, False, "qkv", 512, 512), (HF, 32, True, "shared", 300, 1370),
                                                 (BF, 64, True, "plain", 1024, 512), (HF, 64, False, "plain", 200, 130)])
def test_problem_bits_do_not_depend_on_the_batch(cuda, dt, D, vt, layout, Lq, Lk):
    """The DiT's claim 'a batch of N == N single samples' at the attention: the same problem in a (3, 2) batch and alone gives the same bits --
    for the one-wave kernel, the streaming kernel and (no fallback on this data) the K/V-resident one, in the DiT's layouts."""
    H = 2
    big = _dense(dt, D, vt, "both", None, layout, 3, 2, H, Lq, Lk, 11, cuda)
    launch, oidx = _run_dense(big, dt, D, vt, None, 3, 2, H, Lq, Lk)
    launch()
    torch.cuda.synchronize()
    out_big = big["obuf"][oidx.to(cuda)]
    for o, i in ((0, 0), (2, 1), (1, 0)):
        one = _reload(dict(qh=big["qh"][o:o + 1, i:i + 1], kh=big["kh"][o:o + 1, i:i + 1], vh=big["vh"][o:o + 1, i:i + 1], gq=big["gq"],
                           gk=big["gk"]), dt, D, vt, H, Lq, Lk, cuda)
        l1, oi1 = _run_dense(one, dt, D, vt, None, 1, 1, H, Lq, Lk)
        l1()
        torch.cuda.synchronize()
        assert torch.equal(_bits(one["obuf"][oi1.to(cuda)][0, 0]), _bits(out_big[o, i])), f"problem ({o}, {i}) differs from its batch of 6"


def _reload(c, dt, D, vt, H, Lq, Lk, dev):
    """c with its device views rebuilt from its host operands (plain layout, one problem)."""
    n = _dense(dt, D, vt, "none", None, "plain", 1, 1, H, Lq, Lk, 0, dev)
    row = H * (D + 8)
    q_st, k_st, v_st, _ = n["st"]
    qb, kb, vb = n["qd"].cpu(), n["kd"].cpu(), n["vd"].cpu()
    qb[_idx(0, q_st, 1, 1, Lq, H, D)] = c["qh"]
    kb[_idx(0, k_st, 1, 1, Lk, H, D)] = c["kh"]
    if vt:
        vb[_idx(0, (v_st[0], v_st[1], 1, v_st[3], v_st[2]), 1, 1, Lk, H, D)] = c["vh"].contiguous()
    else:
        vb[_idx(0, v_st, 1, 1, Lk, H, D)] = c["vh"]
    n.update(qh=c["qh"], kh=c["kh"], vh=c["vh"], gq=c["gq"], gk=c["gk"], qd=qb.to(dev), kd=kb.to(dev), vd=vb.to(dev))
    return n


@pytest.mark.parametrize("dt,D,vt,Lk", [(BF, 32, False, 1370), (HF, 64, True, 512), (BF, 64, False, 200)])
def test_rows_do_not_depend_on_their_q_block(cuda, dt, D, vt, Lk):
    """A query row's bits do not depend on which q-block (streaming: 128 rows; K/V-resident: 32-row waves, 256-row passes) it falls in:
    the same 300 rows launched with 64 other rows in front of them."""
    H, Lq = 2, 300
    a = _dense(dt, D, vt, "both", None, "plain", 1, 1, H, Lq + 64, Lk, 21, cuda)
    la, ia = _run_dense(a, dt, D, vt, None, 1, 1, H, Lq + 64, Lk)
    la()
    b = dict(a)
    b["qh"] = a["qh"][:, :, 64:]
    b = _reload(b, dt, D, vt, H, Lq, Lk, cuda)
    lb, ib = _run_dense(b, dt, D, vt, None, 1, 1, H, Lq, Lk)
    lb()
    torch.cuda.synchronize()
    assert torch.equal(_bits(a["obuf"][ia.to(cuda)][0, 0, 64:]), _bits(b["obuf"][ib.to(cuda)][0, 0])), \
        f"path {_path(D, vt, False, Lq, Lk)} / {_path(D, vt, False, Lq + 64, Lk)}"


# ---- the tiled K/V caches (csrc/attn_xt.hip: attention_tiled, head_dim 32; csrc/attn_xt64.hip: attention_tiled64, head_dim 64) ------------

# (path, dtype, n_outer, n_inner, H, Lq, Lk, shared set, key order, gains, fp32 out, force_exact, bounded)
TILED = [
    ("xt", BF, 2, 3, 2, 300, 1370, True, True, True, False, False, False),
    ("xt", HF, 1, 2, 2, 257, 4097, True, True, True, True, False, False),
    ("xt", HF, 2, 2, 1, 129, 77, False, False, False, False, False, False),
    ("xt", BF, 1, 2, 2, 64, 1370, False, False, True, True, True, False),
    ("xt", HF, 1, 1, 2, 513, 63, True, False, True, False, False, True),
    ("xt", HF, 1, 2, 2, 256, 1370, True, True, True, False, True, False),
    ("xt64", BF, 1, 3, 2, 2049, 512, False, False, False, False, False, False),
    ("xt64", HF, 1, 2, 2, 300, 33, False, False, False, False, False, False),
    ("xt64", HF, 2, 1, 2, 65, 447, False, False, False, False, True, False),
    ("xt64", BF, 1, 1, 2, 1, 64, False, False, False, False, True, False),
]


@pytest.mark.parametrize("path,dt,n_outer,n_inner,H,Lq,Lk,shared,ordered,gains,f32,exact,bounded", TILED)
def test_tiled_cache_attention_elementwise(cuda, path, dt, n_outer, n_inner, H, Lq, Lk, shared, ordered, gains, f32, exact, bounded):
    """attention_tiled / attention_tiled64 against attn_ref.model_tiled: bound, guard band, NaN-padded q, repeat bits, the fallback counter at
    0 on ordinary data (force_exact: the exact model); attn_xt: gvf_attn_tiled_fwd_pf with a prefetch range and gvf_attn_tiled_fwd give the
    same bits; one problem of the batch launched alone gives the same bits."""
    from gvfdiffusion_amd.ops.dit_ops import _p, _s4, _stream, dt_code
    D = 32 if path == "xt" else 64
    g = torch.Generator().manual_seed(Lq * 3 + Lk)
    n_sets = n_outer if shared else n_outer * n_inner
    kso, ksi = (1, 0) if shared else (n_inner, 1)
    qh = (1.5 * torch.randn((n_outer, n_inner, Lq, H, D), generator=g)).to(dt)
    kv = torch.randn((n_sets * Lk, 2 * H * D), generator=g)
    kv[:, :H * D] *= 1.5
    gq = (1.0 + 0.2 * torch.randn((H, D), generator=g)) if gains else None
    gk = (1.0 + 0.2 * torch.randn((H, D), generator=g)) if gains else None
    kvd = kv.to(cuda)
    order = dit_ops.key_order_by_norm(kvd, n_sets, Lk, H, 0) if ordered else None
    if path == "xt":
        kt, vt = dit_ops.attention_pack_kv(kvd, n_sets, Lk, H, 0, H * D, gamma_k=None if gk is None else gk.to(cuda), dtype=dt, key_order=order)
    else:
        kt, vt = dit_ops.attention_pack_kv64(kvd, n_sets, Lk, H, 0, H * D, dtype=dt)
    row = H * (D + 8)
    q_st = (n_inner * (Lq + 1) * row, (Lq + 1) * row, row, D + 8)
    qb = torch.full((n_outer * n_inner * (Lq + 1) * row,), float("nan"), dtype=dt)
    qb[_idx(0, q_st, n_outer, n_inner, Lq, H, D)] = qh
    qd = qb.to(cuda)
    o_row = H * D + 8
    o_st = (n_inner * (Lq + 3) * o_row, (Lq + 3) * o_row, o_row, D)
    odt = torch.float32 if f32 else dt
    nout = n_outer * n_inner * (Lq + 3) * o_row
    obuf = (torch.full((nout,), float("nan"), dtype=odt) if f32 else torch.full((nout,), SENTINEL16, dtype=torch.int16).view(dt)).to(cuda)
    fb = torch.zeros(1, dtype=torch.int32, device=cuda)
    gqd = None if gq is None else gq.to(cuda)

    def launch(q=qd, out=obuf, no=n_outer, ni=n_inner, k_t=kt, v_t=vt, so=kso, si=ksi, prefetch=None):
        if path == "xt":
            dit_ops.attention_tiled(q, k_t, v_t, out, no, ni, Lq, Lk, H, q_st, o_st, so, si, gamma_q=gqd, force_exact=exact, fallback_counter=fb,
                                    bounded=bounded, prefetch=prefetch)
        else:
            dit_ops.attention_tiled64(q, k_t, v_t, out, no, ni, Lq, Lk, H, q_st, o_st, so, si, force_exact=exact, fallback_counter=fb)
    oidx = _idx(0, o_st, n_outer, n_inner, Lq, H, D)
    what = f"{path} {str(dt)[6:]} {n_outer}x{n_inner}x{H} Lq{Lq} Lk{Lk} shared={shared} ordered={ordered} gains={gains} f32={f32} exact={exact} bounded={bounded}"
    out = _launch_checked(obuf, oidx, launch, what)
    if not exact:
        assert int(fb.item()) == 0, f"{what}: {int(fb.item())} workgroups fell back on ordinary data"
    # reference, per (outer, inner, head) problem, keys in the cache's order
    kk = kv[:, :H * D].view(n_sets, Lk, H, D).permute(0, 2, 1, 3)
    vv = kv[:, H * D:].view(n_sets, Lk, H, D).permute(0, 2, 1, 3)
    if order is not None:
        o_ = order.cpu().long()[..., None].expand(n_sets, H, Lk, D)
        kk, vv = kk.gather(2, o_), vv.gather(2, o_)
    sets = (torch.arange(n_outer)[:, None] * kso + torch.arange(n_inner)[None, :] * ksi).reshape(-1)
    q, gq_p, _ = _problems(qh, gq, None)
    k = kk[sets].reshape(-1, Lk, D)
    v = vv[sets].reshape(-1, Lk, D)
    gk_p = None if gk is None else gk[None].expand(n_outer * n_inner, H, D).reshape(-1, D)
    ref, bnd = A.model_tiled(q, k, v, path, gq=gq_p, gk=gk_p, shift=(dt == torch.float16 and not bounded), out_f32=f32,
                             fallback=True if exact else None)
    _check(_problems(out, None, None)[0], ref, bnd, what, path)
    if path == "xt":                               # the prefetching launch and the plain entry point: the same bits
        pf = torch.zeros(1 << 20, dtype=torch.float32, device=cuda)
        o2 = obuf.clone()
        launch(out=o2, prefetch=pf)
        o3 = obuf.clone()
        _lib_check = dit_ops._lib.check
        _lib_check(dit_ops._lib.lib().gvf_attn_tiled_fwd(dt_code(dt), _p(qd), _p(kt), _p(vt), _p(o3), n_outer, n_inner, Lq, Lk, H, _s4(q_st),
                                                         _s4(o_st), kso, ksi, _p(gqd), int(f32), int(exact) | (2 if bounded else 0), _p(fb),
                                                         _stream(qd)), "gvf_attn_tiled_fwd")
        torch.cuda.synchronize()
        assert torch.equal(_bits(o2), _bits(obuf)) and torch.equal(_bits(o3), _bits(obuf)), f"{what}: _pf / plain entry point differ"
    # the last problem of the batch alone (its set and q rows as the base): the same bits
    o_l, i_l = n_outer - 1, n_inner - 1
    set_bytes = H * ((Lk + 63) // 64) * (4096 if path == "xt" else 8192)
    s_l = o_l * kso + i_l * ksi
    alone = obuf.clone()
    launch(q=qd[o_l * q_st[0] + i_l * q_st[1]:], out=alone, no=1, ni=1, k_t=kt[s_l * set_bytes:], v_t=vt[s_l * set_bytes:], so=0, si=0)
    torch.cuda.synchronize()
    assert torch.equal(_bits(alone[oidx[0, 0].to(cuda)]), _bits(obuf[oidx[o_l, i_l].to(cuda)])), f"{what}: a problem alone differs from its batch"


def test_worst_ratio_per_path_summary(cuda):
    """Prints the worst |err| / bound seen per path in this process (runs last in file order)."""
    print("worst |err| / bound per path:", {k: round(v, 3) for k, v in sorted(WORST.items())})


def test_kvres_modes_in_child_processes(cuda):
    """This file again in two child processes, one at a time, with GVF_ATTN_KVRES=0 (the K/V-resident kernel off: its shapes on the streaming
    kernel) and =2 (it takes every call with Lk <= 512 and Lq >= 128, varlen with max_Lq >= 128 included); each case's bound follows _path."""
    if CHILD:
        return
    for mode in ("0", "2"):
        r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-s", "-m", "gpu", "-p", "no:cacheprovider", os.path.abspath(__file__)],
                           cwd=ROOT, env=dict(os.environ, GVF_ATTN_CONFORMANCE_CHILD="1", GVF_ATTN_KVRES=mode), capture_output=True, text=True,
                           timeout=600)
        lines = r.stdout.strip().splitlines()
        print(f"GVF_ATTN_KVRES={mode}:", next((l.lstrip(".") for l in lines if "worst |err|" in l), ""), lines[-1] if lines else "")
        assert r.returncode == 0, f"GVF_ATTN_KVRES={mode}:\n" + r.stdout[-3000:] + r.stderr[-2000:]
