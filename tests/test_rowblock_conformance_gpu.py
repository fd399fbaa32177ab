"""Element-wise conformance of the row-block launch (csrc/rowblock.hip, gvf_rowblock_fused) against the float64 reference of
tests/rowblock_ref.py, stage by stage from the kernel's own observable values.  Every case checks, for bf16 and fp16, (a) every element of
x, hb_out and out3 within the bound of its stage, (b) guard bands: the outputs are views inside larger buffers pre-filled with NaN / a 16-bit
sentinel and the rows around them stay untouched, the K / V^T tile buffers stay untouched behind their last tile, (c) operand padding holds
NaN wherever the contract lets it (columns of `a` past K1, rows of `a` past M, columns of the modulation table outside the slices in use,
rows of x_in past groups * period), (d) the same bits on a second launch, and prints (e) the worst |err| / bound per stage and the share of
LayerNorm outputs whose interval spans two 16-bit values.  The launch forms of DiT._blocks_rowblock at the released shape (N = 512: to_qkv of
the spatial self attention writes K / V^T as tiles) are in the matrix: `in` = in_tiles_released (input_layer + position embedding of period
512 + adaLN + tiles; two samples of three frames rather than one of 24), s2 / s3 / s4 = s2_adaln_qkv, s3_affine_q, s4_no_gate (a few
blocks) and s2_full (M = 12288), s23 = the temporal launch at B = 1, T = 24, N = 512, s5 = s5_full (M = 12288, hidden 2048, tiles of 512
keys), the last MLP = s5_last; the other in_* / s5_* rows are the row-major forms that smaller N launches.  MLP and temporal launches are run
twice: with a zero second gate, which exposes their phase-1 stream bit for bit, and in full, whose second update is held to the propagated
bound from that stream.  Two probe launches resolve what the propagated bounds cannot: the hidden units (mlp.2 = identity) and the attention
output (rows with an unambiguous LayerNorm output, to_out = identity; to_qkv a signed permutation, or eight entries per row so that the rounding of
q / k / v is held too).  Invariance tests compare bits, not bounds; refusals are host-side
return codes.  The whole file takes under 30 s on an MI355X, most of it the float64 references of the M = 12288 cases (s2_full, s5_full and the temporal one, in both types)."""
import ctypes

import pytest
import torch

import rowblock_ref as R
from gvfdiffusion_amd import _lib
from gvfdiffusion_amd.ops import dit_ops

pytestmark = pytest.mark.gpu
C, H = 512, 16
SENTINEL16 = 0x7E5A                  # as tests/test_gemm_conformance_gpu.py
DTYPES = [torch.bfloat16, torch.float16]
GUARD = 8                            # rows in front of and behind every output view


def _bits(t):
    return t.view(torch.int16) if t.element_size() == 2 else (t.view(torch.int32) if t.element_size() == 4 else t)


def _guarded(M, n, dt, dev):
    """(buffer, view): an (M, n) contiguous view with GUARD sentinel rows on either side."""
    if dt == torch.float32:
        buf = torch.full((M + 2 * GUARD, n), float("nan"), dtype=dt, device=dev)
    else:
        buf = torch.full((M + 2 * GUARD, n), SENTINEL16, dtype=torch.int16, device=dev).view(dt)
    return buf, buf[GUARD:GUARD + M]


def _guards_intact(buf, M, what):
    b = _bits(buf)
    ref = _bits(torch.full((1,), float("nan"), dtype=buf.dtype)) if buf.dtype == torch.float32 else torch.tensor([SENTINEL16], dtype=torch.int16)
    ok = bool((b[:GUARD] == ref.to(b.device)).all()) and bool((b[GUARD + M:] == ref.to(b.device)).all())
    assert ok, f"{what}: a store outside the rows of the launch"


class Dev:
    """Device copies of a rowblock_ref case with NaN in every padding the contract allows."""

    def __init__(self, d, dev):
        self.d, self.dev = d, dev
        M, dt = d["M"], d["dt"]
        nan = float("nan")
        self.a = None
        if d.get("a") is not None:
            K1 = d["a"].shape[1]
            lda = K1 + d.get("lda_pad", 0)
            buf = torch.full((M + 3, lda), nan, dtype=dt, device=dev)
            buf[:M, :K1] = d["a"].to(dev)
            self.a = buf[:M, :K1]
        mod = d.get("mod")
        self.mod_dev = None if mod is None else torch.full(mod.shape, nan, device=dev)
        self.mod_ld = 0

        def grouped(t):                              # a (groups, >= 512) vector: a view of the modulation table, or a table of its own
            if t is None:
                return None
            if mod is not None and t.untyped_storage().data_ptr() == mod.untyped_storage().data_ptr():
                off = t.storage_offset()
                self.mod_dev[:, off:off + C] = mod[:, off:off + C].to(dev)
                v = self.mod_dev[:, off:]
            else:
                v = t.to(dev)
            assert self.mod_ld in (0, v.stride(0))
            self.mod_ld = v.stride(0)
            return v

        def ln(l):
            l = l or {}
            return dict(ln_w=self.to(l.get("ln_w")), ln_b=self.to(l.get("ln_b")), shift=grouped(l.get("shift")), scale=grouped(l.get("scale")))

        self.gate1, self.gate_m = grouped(d.get("gate1")), grouped(d.get("gate_m"))
        self.ln1, self.ln2 = ln(d.get("ln1")), ln(d.get("ln2"))
        self.zero_gate = None
        self.temporal = None
        if d.get("T"):
            self.t_gate, self.t_ln = grouped(d.get("t_gate")), ln(d.get("t_ln"))
            self.temporal = dict(frames=d["T"], stride=d["N"], b_qkv=self.to(d.get("bqkv")), gamma_q=self.to(d.get("gq")), gamma_k=self.to(d.get("gk")),
                                 b_out=self.to(d.get("bout")), gate=self.t_gate, ln=self.t_ln, scale=d.get("t_scale"))
        if d.get("hidden") or d.get("T"):
            self.zero_gate = torch.zeros((M // d["rpg"], max(self.mod_ld, C)), device=dev)
            self.mod_ld = self.zero_gate.stride(0)
        self.b1, self.b3, self.bfc1, self.bfc2 = (self.to(d.get(k)) for k in ("b1", "b3", "bfc1", "bfc2"))
        self.in_x, self.in_wt, self.in_b = (self.to(d.get(k)) for k in ("in_x", "in_wt", "in_b"))
        self.x_in = None
        if d.get("x_in") is not None:
            buf = torch.full((d["x_in"].shape[0] + 5, C), nan, device=dev)
            buf[:d["x_in"].shape[0]] = d["x_in"].to(dev)
            self.x_in = buf[:d["x_in"].shape[0]]
        w1 = self.to(d.get("w1"))
        mlp = (self.to(d["wfc1"]), self.to(d["wfc2"])) if d.get("hidden") else None
        self.w3 = self.to(d.get("w3"))
        tw = (self.to(d["wqkv"]), self.to(d["wout"])) if d.get("T") else None
        self.stream = dit_ops.rowblock_pack_stream(w1, mlp=mlp, w3=self.w3, temporal=tw)
        self.stream_no3 = dit_ops.rowblock_pack_stream(w1, mlp=mlp, w3=None) if (w1 is not None or mlp is not None) else None

    def to(self, t):
        return None if t is None else t.to(self.dev).contiguous()

    def launch(self, hb=False, out3=True, zero_gate_m=False, kv=None, what=""):
        """One launch in guarded buffers, its guard bands checked, then a second launch compared bit for bit.  Returns CPU copies."""
        d, dev = self.d, self.dev
        M, dt = d["M"], d["dt"]
        out3 = out3 and self.w3 is not None
        xbuf, x = _guarded(M, C, torch.float32, dev)
        n3 = C if kv is not None else (self.w3.shape[0] if out3 else 0)
        obuf, o = _guarded(M, n3, dt, dev) if out3 else (None, None)
        hbuf, h = _guarded(M, C, dt, dev) if hb else (None, None)
        kw = dict(b1=self.b1, gate1=self.gate1, ln1=self.ln1, mod_ld=self.mod_ld, rows_per_group=d["rpg"], eps=d.get("eps", 1e-6), b3=self.b3 if out3 else None,
                  out3=o, hb_out=h, x_in=self.x_in, x_in_period=d.get("period", 0), in_x=self.in_x, in_wt=self.in_wt, in_b=self.in_b, dtype=dt)
        if d.get("hidden"):
            kw.update(mlp_bias=(self.bfc1, self.bfc2), hidden=d["hidden"], gate_m=self.zero_gate if zero_gate_m else self.gate_m, ln2=self.ln2)
        if self.temporal is not None:
            kw.update(temporal=dict(self.temporal, gate=self.zero_gate if zero_gate_m else self.t_gate))
        if kv is not None:
            kw.update(kv_tiles=(kv["kt"], kv["vt"]), kv_L=kv["L"], gamma_k=kv.get("gamma_k"), kv_group_rows=kv.get("group_rows", 0))
        stream = self.stream if out3 else self.stream_no3
        x_init = d["x0"].to(dev) if self.x_in is None else torch.full((M, C), 12345.0, device=dev)      # x_in: x is only written

        def go():
            x.copy_(x_init)
            dit_ops.rowblock_fused(self.a, stream, x, **kw)
            torch.cuda.synchronize()

        go()
        first = [t.clone() for t in (x, o, h) if t is not None] + ([kv["kt"].clone(), kv["vt"].clone()] if kv is not None else [])
        for buf, name in ((xbuf, "x"), (obuf, "out3"), (hbuf, "hb_out")):
            if buf is not None:
                _guards_intact(buf, M, f"{what} {name}")
        go()
        second = [t for t in (x, o, h) if t is not None] + ([kv["kt"], kv["vt"]] if kv is not None else [])
        assert all(torch.equal(_bits(p), _bits(q)) for p, q in zip(first, second)), f"{what}: a second launch gave other bits"
        return dict(x=x.cpu(), out3=None if o is None else o.cpu(), hb=None if h is None else h.cpu())


def _report(res, what, stages):
    worst = {k: res[k][1] for k in stages if k in res}
    print(f"{what}: worst |err| / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()) +
          (f"; ambiguous LayerNorm outputs {100 * res['amb_share']:.3f} %" if "amb_share" in res else ""))
    for k in stages:
        if k in res:
            n = int(res[k][0].sum())
            rows = res[k][0].any(1).nonzero().flatten().tolist()[:8]
            assert n == 0, f"{what}: {k}: {n} elements outside the bound (worst {res[k][1]:.3g} x), first rows {rows}"


# name -> make_case arguments.  The forms of DiT._blocks_rowblock (model/dit.py) at C = 512, hidden 2048: in (input_layer on the position
# embedding + adaLN + to_qkv), s2 (to_out + gate + adaLN / affine + to_qkv / to_q), s3 (the same with to_q), s4 (no gate, affine), s5 (MLP +
# adaLN of the next block + to_qkv), s5_last (MLP alone).  The rest is pairwise over K1, lda, the optional vectors, M / rows_per_group, N3.
PLAIN_CASES = {
    "in_cin16": dict(M=288, rpg=144, K1=0, in_cin=16, x_in=True, period=48, N3=1536, ln1="adaln"),
    "in_cin4_period16": dict(M=96, rpg=96, K1=0, in_cin=4, x_in=True, period=16, N3=512, ln1="adaln"),
    "in_cin8_no_x_in": dict(M=48, rpg=48, K1=0, in_cin=8, N3=1024, ln1="both"),
    "in_no_bias": dict(M=96, rpg=48, K1=0, in_cin=16, in_b=False, x_in=True, period=48, N3=512, ln1="affine"),
    "s2_adaln_qkv": dict(M=480, rpg=240, K1=512, N3=1536, ln1="adaln", lda_pad=8),
    "s3_affine_q": dict(M=192, rpg=96, K1=512, N3=512, ln1="affine"),
    "s4_no_gate": dict(M=144, rpg=144, K1=512, N3=512, ln1="affine", gate1=False, lda_pad=24),
    "k128_no_b1": dict(M=96, rpg=48, K1=128, N3=1024, ln1="both", b1=False, lda_pad=8),
    "k256_no_ln": dict(M=48, rpg=48, K1=256, N3=512, ln1="none", b3=False),
    "k384_hb_only": dict(M=240, rpg=48, K1=384, N3=0, ln1="adaln", lda_pad=16),
    "k0_adversarial": dict(M=96, rpg=48, K1=0, N3=512, ln1="both", adv=True),
    "k0_adversarial_plain_ln": dict(M=96, rpg=48, K1=0, N3=512, ln1="none", adv=True),
    "k128_adversarial": dict(M=144, rpg=48, K1=128, N3=512, ln1="adaln", adv=True),
    "s2_full": dict(M=12288, rpg=12288, K1=512, N3=1536, ln1="adaln"),
    # `in` as the released shape launches it: input_layer (16 channels, bias) on the position embedding broadcast with period N = 512 over the
    # frames of a sample, adaLN, to_qkv with q row-major and K / V^T as tiles of kv_L = N keys with the RMS gain (three frames, two samples)
    "in_tiles_released": dict(M=3072, rpg=1536, K1=0, in_cin=16, x_in=True, period=512, N3=1536, ln1="adaln", kv=(512, True)),
}


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("name", list(PLAIN_CASES))
def test_plain_launch_elementwise(cuda, dt, name):
    kw = dict(PLAIN_CASES[name])
    tiles = kw.pop("kv", None)
    d = R.make_case(dt, seed=21, **kw)
    D = Dev(d, cuda)
    what = f"rowblock {name} {dt}"
    out = D.launch(hb=True, what=what)
    _report(R.check_plain(d, out["x"], out["hb"], out["out3"]), what, ("x", "hb", "out3"))
    if d.get("w3") is not None:                   # the same launch without hb_out: the same bits
        lean = D.launch(hb=False, what=what + " (no hb_out)")
        assert torch.equal(_bits(lean["x"]), _bits(out["x"])) and torch.equal(_bits(lean["out3"]), _bits(out["out3"]))
    if tiles is not None:                         # the form the DiT launches: the same rows as tiles
        _check_tiles(D, out, tiles[0], tiles[1], 0, what + " (K / V^T tiles)")


MLP_CASES = {
    "s5_next_qkv": dict(M=192, rpg=96, K1=512, hidden=2048, N3=1536, ln1="adaln", ln2="adaln", gate1=False),
    "s5_last": dict(M=144, rpg=144, K1=512, hidden=2048, N3=0, ln1="adaln", gate1=False),
    "h512_both": dict(M=48, rpg=48, K1=128, hidden=512, N3=512, ln1="both", ln2="affine", lda_pad=8),
    "h1024_hb_only": dict(M=96, rpg=48, K1=256, hidden=1024, N3=0, ln1="affine", ln2="both", want_hb=True),
    "h1536_no_ln2": dict(M=240, rpg=240, K1=384, hidden=1536, N3=1024, ln1="adaln", ln2="none", b1=False),
    "h2048_adversarial": dict(M=96, rpg=48, K1=512, hidden=2048, N3=512, ln1="adaln", ln2="adaln", adv=True),
    # `s5` as the released shape launches it: the MLP, adaLN of the next block, its to_qkv with K / V^T as tiles of 512 keys with the RMS gain
    "s5_full": dict(M=12288, rpg=12288, K1=512, hidden=2048, N3=1536, ln1="adaln", ln2="adaln", gate1=False, kv=(512, True)),
}


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("name", list(MLP_CASES))
def test_mlp_launch_elementwise(cuda, dt, name):
    kw = dict(MLP_CASES[name])
    want_hb, tiles = kw.pop("want_hb", False), kw.pop("kv", None)
    d = R.make_case(dt, seed=23, **kw)
    D = Dev(d, cuda)
    what = f"rowblock MLP {name} {dt}"
    has3 = d.get("w3") is not None
    x1 = D.launch(hb=False, out3=False, zero_gate_m=True, what=what + " (zero gate)")["x"]      # the phase-1 stream, bit for bit
    assert torch.isfinite(x1).all(), f"{what}: a zero gate_m left a non-finite stream: the MLP interior is not finite"
    out = D.launch(hb=has3 or want_hb, what=what)
    res = R.check_mlp(d, x1, out["x"], out["hb"], out["out3"])
    _report(res, what + f" (median bound of the MLP update {res['x_bound_median']:.1e})", ("x1", "x", "hb", "out3"))
    if has3:
        lean = D.launch(hb=False, what=what + " (no hb_out)")
        assert torch.equal(_bits(lean["x"]), _bits(out["x"])) and torch.equal(_bits(lean["out3"]), _bits(out["out3"]))
    if tiles is not None:
        _check_tiles(D, out, tiles[0], tiles[1], 0, what + " (K / V^T tiles)")


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
def test_hidden_unit_probe(cuda, dt):
    """x = 0, no closing projection, hidden = 512, Wfc2 = identity, b_fc2 = 0, gate_m = 1: the stream comes out as the 16-bit hidden units."""
    d = R.make_probe(dt)
    out = Dev(d, cuda).launch(hb=False, out3=False, what=f"hidden-unit probe {dt}")
    bad, worst = R.check_hidden_probe(d, out["x"])
    print(f"hidden-unit probe {dt}: worst |err| / bound {worst:.3f}, |h| from {float(out['x'].abs().min()):.1e} to {float(out['x'].abs().max()):.2f}")
    assert torch.equal(out["x"].to(dt).float(), out["x"]), "the probe's stream holds values that are not 16-bit"
    assert int(bad.sum()) == 0, f"{int(bad.sum())} hidden units outside the bound (worst {worst:.3g} x), rows {bad.any(1).nonzero().flatten().tolist()[:8]}"


def _check_tiles(D, twin, L, rms, kvg, what):
    """The tile-writing form of a launch whose row-major twin (out3 = [q | k | v]) has just been held to the fp64 bound: q and x bit-equal to the
    twin's, the K / V^T tiles bit-equal to attention_pack_kv of the twin's k and v columns, nothing written behind the last key set."""
    d, cuda = D.d, D.dev
    M, rpg = d["M"], d["rpg"]
    g = torch.Generator().manual_seed(L + M)
    gk = (1 + 0.2 * torch.randn((C,), generator=g)).to(cuda) if rms else None
    qkv = twin["out3"].to(cuda)
    groups = M // rpg
    keys = qkv if not kvg else qkv.view(groups, rpg, 3 * C)[:, :kvg].reshape(groups * kvg, 3 * C).contiguous()
    n_sets = keys.shape[0] // L
    kt_ref, vt_ref = dit_ops.attention_pack_kv(keys, n_sets, L, H, C, 2 * C, gamma_k=gk)
    nbytes, extra = kt_ref.numel(), 2 * 4096
    kv = dict(kt=torch.full((nbytes + extra,), 0xAB, dtype=torch.uint8, device=cuda), vt=torch.full((nbytes + extra,), 0xAB, dtype=torch.uint8, device=cuda),
              L=L, gamma_k=gk, group_rows=kvg)
    out = D.launch(hb=False, kv=kv, what=what)
    assert torch.equal(_bits(out["out3"]), _bits(twin["out3"][:, :C])), f"{what}: q differs from the row-major launch"
    assert torch.equal(_bits(out["x"]), _bits(twin["x"]))
    for name, t, ref in (("K", kv["kt"], kt_ref), ("V^T", kv["vt"], vt_ref)):
        assert torch.equal(t[:nbytes], ref), f"{what}: {name} tiles differ in {(t[:nbytes] != ref).sum().item()} bytes"
        assert bool((t[nbytes:] == 0xAB).all()), f"{what}: a {name} tile written behind the last key set"


# (M, rows_per_group, kv_L, gains, kv_group_rows, MLP in front)
KV_CASES = [(192, 192, 64, True, 0, False), (384, 384, 128, False, 0, False), (1536, 1536, 512, True, 0, True), (480, 240, 64, True, 192, False),
            (576, 288, 128, False, 256, True)]


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("M,rpg,L,rms,kvg,mlp", KV_CASES)
def test_tiled_kv_epilogue_elementwise(cuda, dt, M, rpg, L, rms, kvg, mlp):
    """The K / V^T tiles == attention_pack_kv of the row-major out3 of a twin launch, bit for bit; that twin's out3 is what is held to the fp64
    bound.  Tiles behind the last key set stay untouched; with kv_group_rows the padding rows of a group write no tile.  (The two forms the DiT
    launches with tiles at the released shape -- `in` and `s5` -- are PLAIN_CASES["in_tiles_released"] and MLP_CASES["s5_full"].)"""
    d = R.make_case(dt, seed=29, M=M, rpg=rpg, K1=512, hidden=512 if mlp else 0, N3=1536, ln1="adaln", ln2="affine")
    D = Dev(d, cuda)
    what = f"rowblock K/V tiles M{M} L{L} group rows {kvg} {dt}"
    twin = D.launch(hb=True, what=what + " (row-major twin)")
    if mlp:
        x1 = D.launch(hb=False, out3=False, zero_gate_m=True, what=what)["x"]
        _report(R.check_mlp(d, x1, twin["x"], twin["hb"], twin["out3"]), what, ("x1", "x", "hb", "out3"))
    else:
        _report(R.check_plain(d, twin["x"], twin["hb"], twin["out3"]), what, ("x", "hb", "out3"))
    _check_tiles(D, twin, L, rms, kvg, what)


# (B, T, N, gains, adaLN + gates, the closing LayerNorm t_ln).  T: every divisor of 48 the launcher accepts; N: whole blocks (a multiple of 48 / T) and phantom tokens in the last
# block of a group; (1, 24, 512): the released shape, DiT._blocks_rowblock's s23 launch; (2, 16, 9) / (1, 16, 96): padded groups as
# tests/test_rowblock_temporal_gpu.py::test_temporal_section_on_padded_groups has them
TEMPORAL_CASES = [(1, 24, 512, True, True, "affine"), (2, 24, 6, True, True, "both"), (3, 12, 16, False, False, "affine"), (1, 48, 7, True, False, "adaln"),
                  (2, 16, 9, True, True, "affine"), (1, 1, 96, True, True, "none"), (2, 8, 30, False, True, "adaln"), (3, 2, 24, True, False, "affine"),
                  (1, 2, 25, False, True, "both"), (2, 3, 16, True, True, "affine"), (1, 3, 50, False, False, "none"), (2, 4, 13, True, False, "both"),
                  (1, 6, 64, True, True, "adaln"), (3, 6, 11, False, True, "affine"), (1, 16, 96, True, False, "affine"), (1, 12, 5, True, True, "none")]


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("B,T,N,rms,adaln,t_ln", TEMPORAL_CASES)
def test_temporal_launch_elementwise(cuda, dt, B, T, N, rms, adaln, t_ln):
    d = R.make_temporal(dt, B, T, N, rms=rms, adaln=adaln, seed=43, gate=adaln, t_ln=t_ln)
    D = Dev(d, cuda)
    what = f"rowblock temporal B{B} T{T} N{N} {dt}"
    x1 = D.launch(zero_gate_m=True, what=what + " (zero gate)")["x"]      # the phase-1 stream, bit for bit
    assert torch.isfinite(x1).all(), f"{what}: a zero t_gate left a non-finite stream: the attention interior is not finite"
    out = D.launch(what=what)
    res = R.check_temporal(d, x1, out["x"], out["out3"])
    _report(res, what + f" (median bound of the temporal update {res['x_bound_median']:.1e})", ("x1", "x", "out3"))


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("B,T,N,rms", [(1, 24, 8, True), (2, 16, 5, True), (1, 48, 3, False), (2, 6, 11, True), (1, 3, 20, False), (1, 1, 48, True), (1, 8, 9, True),
                                       (2, 12, 7, False), (1, 4, 24, True), (1, 2, 30, True)])
@pytest.mark.parametrize("real_qkv", [False, True], ids=["permutation", "projection"])
def test_attention_output_probe(cuda, dt, B, T, N, rms, real_qkv):
    """Rows whose LayerNorm output is unambiguous, Wout = identity, gate1 = 0, t_gate = 1: x - x0 is the 16-bit attention output.  With to_qkv =
    signed permutations q, k, v are exact and P, l, o are held to the fp32 softmax arithmetic alone; with a to_qkv of eight entries per row
    they are genuinely rounded and their own rounding is held too, at a width of one or two steps of o (rowblock_ref.check_attention_probe)."""
    d = R.make_temporal_probe(dt, B, T, N, rms=rms, real_qkv=real_qkv)
    out = Dev(d, cuda).launch(what=f"attention probe T{T} N{N} {dt}")
    (bad, worst), o_share, ln_share = R.check_attention_probe(d, out["x"])
    print(f"attention probe B{B} T{T} N{N} {dt} real to_qkv {real_qkv}: worst |err| / bound {worst:.3f}; outputs that may hold more than one 16-bit value {100 * o_share:.2f} %")
    assert ln_share == 0.0
    assert int(bad.sum()) == 0, f"{int(bad.sum())} elements outside the bound (worst {worst:.3g} x), grid rows {bad.any(1).nonzero().flatten().tolist()[:8]}"


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("T", [6, 24])
def test_a_tokens_bits_do_not_depend_on_the_tokens_that_share_its_block(cuda, dt, T):
    """Five tokens alone in their group (the rest of their last block: phantom tokens) and the same five tokens as tokens 0 .. 4 of a group of 11,
    with real tokens of other data where the phantom ones were: the same bits in x and out3.  (The tokens keep their place in the block.  A
    token moved to other local rows -- tokens 3 .. 7 of the larger group -- kept its bf16 bits but not its fp16 ones when that was tried on the
    MI355X; the P V product contracts over the block's key slots, so the order of its sum moves with the token.  DiT's batch promise does
    not move tokens.)"""
    one = R.make_temporal(dt, 1, T, 5, seed=47)
    big = R.make_temporal(dt, 1, T, 11, seed=53)
    for k in ("w1", "b1", "wqkv", "bqkv", "wout", "bout", "gq", "gk", "w3", "b3", "mod"):
        big[k].copy_(one[k])
    for k in ("ln_w", "ln_b"):
        big["t_ln"][k].copy_(one["t_ln"][k])
    f, n = torch.meshgrid(torch.arange(T), torch.arange(5), indexing="ij")
    r1, r2 = (f * 5 + n).reshape(-1), (f * 11 + n).reshape(-1)
    for k in ("x0", "a"):
        big[k][r2] = one[k][r1]
    o1, o2 = Dev(one, cuda).launch(what="token alone"), Dev(big, cuda).launch(what="token among others")
    for k in ("x", "out3"):
        assert torch.equal(_bits(o2[k][r2]), _bits(o1[k][r1])), f"{k}: a token's bits depend on the tokens that share its block"


# ---- invariance: bits, not bounds ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("hidden", [0, 2048])
def test_a_rows_bits_do_not_depend_on_its_block_group_or_batch(cuda, dt, hidden):
    """The 96 rows of one group (with its modulation vectors) give the same x, hb_out, out3 alone (B = 1), as group 0 and as group 2 of a launch
    of three groups (B = 3, the other groups holding other data), and with their two 48-row blocks exchanged inside the group."""
    one = R.make_case(dt, seed=31, M=96, rpg=96, K1=512, hidden=hidden, N3=512, ln1="adaln", ln2="both")
    ref = Dev(one, cuda).launch(hb=True, what="invariance B=1")
    for pos in (0, 2):
        big = R.make_case(dt, seed=37, M=288, rpg=96, K1=512, hidden=hidden, N3=512, ln1="adaln", ln2="both")
        rows = slice(96 * pos, 96 * pos + 96)
        for k in ("x0", "a"):
            big[k][rows] = one[k]
        big["mod"][pos] = one["mod"][0]
        for k in ("w1", "b1", "w3", "b3", "wfc1", "wfc2", "bfc1", "bfc2"):
            if k in one:
                big[k].copy_(one[k])
        for k in ("ln_w", "ln_b"):
            if hidden:
                big["ln2"][k].copy_(one["ln2"][k])
        out = Dev(big, cuda).launch(hb=True, what=f"invariance B=3 group {pos}")
        for k in ("x", "hb", "out3"):
            assert torch.equal(_bits(out[k][rows]), _bits(ref[k])), f"{k}: a row's bits depend on the group it sits in (group {pos} of 3)"
    sw = dict(one)
    perm = torch.cat([torch.arange(48, 96), torch.arange(0, 48)])
    sw["x0"], sw["a"] = one["x0"][perm].clone(), one["a"][perm].clone()
    out = Dev(sw, cuda).launch(hb=True, what="invariance blocks exchanged")
    for k in ("x", "hb", "out3"):
        assert torch.equal(_bits(out[k][perm]), _bits(ref[k])), f"{k}: a row's bits depend on the block it sits in"


# ---- refusals: host-side return codes, nothing is launched --------------------------------------------------------------------------------

def test_launcher_refuses_what_the_kernel_cannot_handle(cuda):
    """One refusal per GVF_EINVAL branch of rowblock_launch (csrc/rowblock.hip) beyond those tests/test_dit_gpu.py, tests/test_capi_symbols.py
    and tests/test_rowblock_temporal_gpu.py already exercise.  Every call is refused on the host, before anything is launched: the outputs
    keep their sentinel.  (Every buffer is large enough for the largest M named here.)"""
    dt = torch.bfloat16
    d = R.make_case(dt, seed=41, M=192, rpg=48, K1=128, hidden=512, N3=1536, ln1="adaln", ln2="adaln")
    dd = {k: (v.to(cuda) if torch.is_tensor(v) else v) for k, v in d.items()}
    mod, ld = dd["mod"], dd["mod"].stride(0)
    lw, lb = torch.ones(C, device=cuda), torch.zeros(C, device=cuda)
    s_plain = dit_ops.rowblock_pack_stream(dd["w1"], w3=dd["w3"])
    s_mlp = dit_ops.rowblock_pack_stream(dd["w1"], mlp=(dd["wfc1"], dd["wfc2"]), w3=dd["w3"])
    s_k0 = dit_ops.rowblock_pack_stream(None, w3=dd["w3"])
    x, a = dd["x0"].clone(), dd["a"]
    out = torch.full((192, 1536), SENTINEL16, dtype=torch.int16, device=cuda).view(dt)
    hb = torch.full((192, C), SENTINEL16, dtype=torch.int16, device=cuda).view(dt)
    kt = torch.full((4 * H * 4096,), 0xAB, dtype=torch.uint8, device=cuda)
    vt = kt.clone()
    ada = dict(shift=mod[:, C:], scale=mod[:, 2 * C:])
    base = dict(b1=dd["b1"], gate1=mod, ln1=ada, mod_ld=ld, rows_per_group=48, out3=out, b3=dd["b3"])
    k0 = dict(base, b1=None, gate1=None)
    mlp = dict(mlp_bias=(dd["bfc1"], dd["bfc2"]), hidden=512, gate_m=mod[:, 5 * C:], ln2=ada)
    in_kw = dict(in_x=torch.zeros((192, 8), device=cuda), in_wt=torch.zeros((8, C), device=cuda))
    through_the_binding = {
        "lda not a multiple of 8": (torch.zeros((192, 132), dtype=dt, device=cuda)[:, :128], s_plain, base),
        "gate1 without a closing projection": (None, s_k0, dict(base, b1=None)),
        "b1 without a closing projection": (None, s_k0, dict(base, gate1=None)),
        "in_x with 6 channels": (None, s_k0, dict(k0, in_x=torch.zeros((192, 6), device=cuda), in_wt=torch.zeros((6, C), device=cuda))),
        "in_wt not 16-byte aligned": (None, s_k0, dict(k0, in_x=in_kw["in_x"], in_wt=torch.zeros((8 * C + 1,), device=cuda)[1:].view(8, C))),
        "in_b not 16-byte aligned": (None, s_k0, dict(k0, in_b=torch.zeros((C + 1,), device=cuda)[1:], **in_kw)),
        "x_in without a period": (a, s_plain, dict(base, x_in=dd["x0"], x_in_period=0)),
        "x_in with rows_per_group not whole blocks": (a, s_plain, dict(base, gate1=None, ln1=dict(ln_w=lw, ln_b=lb), rows_per_group=40, x_in=dd["x0"], x_in_period=16)),
        "ln_w without ln_b": (a, s_plain, dict(base, ln1=dict(ln_w=lw))),
        "shift without scale": (a, s_plain, dict(base, ln1=dict(shift=mod[:, C:]))),
        "modulation without rows_per_group": (a, s_plain, dict(base, rows_per_group=0)),
        "rows_per_group not whole blocks": (a, s_plain, dict(base, rows_per_group=32)),
        "mod_ld below 512": (a, s_plain, dict(base, mod_ld=256)),
        "MLP with x_in": (a, s_mlp, dict(base, x_in=dd["x0"], x_in_period=48, **mlp)),
        "hidden not a multiple of 512": (a, s_mlp, dict(base, **dict(mlp, hidden=768))),
        "hidden above 2048": (a, s_mlp, dict(base, **dict(mlp, hidden=2560))),
        "N3 above 1536": (a, s_plain, dict(base, out3=torch.empty((192, 2048), dtype=dt, device=cuda))),
        "N3 not a multiple of 512": (a, s_plain, dict(base, out3=torch.empty((192, 768), dtype=dt, device=cuda))),
        "nothing to write": (a, s_plain, dict(base, out3=None, b3=None)),
        "b3 not 16-byte aligned": (a, s_plain, dict(base, b3=torch.zeros((1537,), device=cuda)[1:])),
        "LayerNorm alone (an empty weight stream)": (None, s_k0, dict(ln1=dict(ln_w=lw, ln_b=lb), hb_out=hb)),
    }
    for name, (a_, stream, kw) in through_the_binding.items():
        try:
            dit_ops.rowblock_fused(a_, stream, x, **kw)
        except _lib.GvfError:
            continue
        raise AssertionError(f"accepted: {name}")
    # the branches the Python binding asserts before the library sees them: straight through ctypes
    L = _lib.lib()

    def args(**kw):
        A = dit_ops.RowblockArgs()
        A.dtype, A.a, A.lda, A.K1, A.w, A.x, A.M, A.C = dit_ops.dt_code(dt), a.data_ptr(), 128, 128, s_plain.data_ptr(), x.data_ptr(), 96, C
        A.ln1 = dit_ops.RowblockLn(lw.data_ptr(), lb.data_ptr(), None, None)
        A.out3, A.N3, A.epi3, A.eps = out.data_ptr(), 1536, dit_ops.EPI_STORE_BF16, 1e-6
        for k, v in kw.items():
            setattr(A, k, v)
        return A

    tiles = dict(k_tiles=kt.data_ptr(), v_tiles=vt.data_ptr(), kv_L=64, k_scale=0.25)
    temporal = dict(N3=512, t_frames=24, t_stride=2, rows_per_group=48, t_scale=0.17)
    refused = {
        "C other than 512": args(C=256), "K1 not a multiple of 128": args(K1=96), "K1 above 512": args(K1=640, lda=640), "lda below K1": args(lda=64),
        "null stream of weights": args(w=None), "null x": args(x=None), "null a": args(a=None), "negative M": args(M=-48),
        "in_x with a closing projection": args(in_x=x.data_ptr(), in_wt=x.data_ptr(), in_cin=8),
        "MLP with in_x": args(K1=0, a=None, hidden=512, in_x=x.data_ptr(), in_wt=x.data_ptr(), in_cin=8),
        "null out3": args(out3=None), "another epilogue": args(epi3=dit_ops.EPI_GELU_BF16),
        "K tiles without V tiles": args(k_tiles=kt.data_ptr()),
        "K tiles without N3 = 1536": args(M=192, N3=512, **tiles), "kv_L not a multiple of 64": args(**dict(tiles, kv_L=32)),
        "k_scale not positive": args(M=192, **dict(tiles, k_scale=0.0)),
        "K tiles not 16-byte aligned": args(M=192, **dict(tiles, k_tiles=kt.data_ptr() + 8)),
        "rows not whole key sets": args(M=96, **tiles),
        "kv_group_rows without tiles": args(kv_group_rows=64, rows_per_group=96),
        "kv_group_rows not whole key sets": args(M=192, rows_per_group=96, **dict(tiles, kv_group_rows=96)),
        "kv_group_rows above rows_per_group": args(M=192, rows_per_group=96, **dict(tiles, kv_group_rows=128)),
        "x not 16-byte aligned": args(x=x.data_ptr() + 4), "a not 16-byte aligned": args(a=a.data_ptr() + 8),
        "out3 not 8-byte aligned": args(out3=out.data_ptr() + 2), "hb_out not 8-byte aligned": args(hb_out=hb.data_ptr() + 2),
        "M * 512 beyond 32-bit offsets": args(M=48 * 174763),
        "temporal with hb_out": args(hb_out=hb.data_ptr(), **temporal),
        "temporal with an MLP": args(hidden=512, **temporal),
        "temporal without a closing projection": args(K1=0, a=None, **temporal),
        "temporal scale not positive": args(**dict(temporal, t_scale=0.0)),
        "temporal LayerNorm with ln_w alone": args(t_ln=dit_ops.RowblockLn(lw.data_ptr(), None, None, None), **temporal),
        "temporal gate with mod_ld below 512": args(t_gate=mod.data_ptr(), mod_ld=8, **temporal),
        "unknown dtype": args(dtype=7),
        "in_x with 20 channels": args(K1=0, a=None, in_x=x.data_ptr(), in_wt=x.data_ptr(), in_cin=20),
        "in_x without in_wt": args(K1=0, a=None, in_x=x.data_ptr(), in_cin=8),
        "x_in not 16-byte aligned": args(x_in=x.data_ptr() + 4, x_in_period=48, rows_per_group=48),
        "weight stream not 16-byte aligned": args(w=s_plain.data_ptr() + 8),
        "gamma_q without gamma_k": args(t_gamma_q=lw.data_ptr(), **temporal),
    }
    assert L.gvf_rowblock_fused(None, None) == _lib.GVF_EINVAL, "accepted: a null argument block"
    for name, A in refused.items():
        assert L.gvf_rowblock_fused(ctypes.byref(A), None) == _lib.GVF_EINVAL, f"accepted: {name}"
    assert L.gvf_rowblock_fused(ctypes.byref(args(M=0)), None) == _lib.GVF_OK          # an empty launch is accepted and does nothing
    torch.cuda.synchronize()
    assert bool((_bits(out) == SENTINEL16).all()) and bool((_bits(hb) == SENTINEL16).all()) and torch.equal(x, dd["x0"])
    assert bool((kt == 0xAB).all()) and bool((vt == 0xAB).all())
