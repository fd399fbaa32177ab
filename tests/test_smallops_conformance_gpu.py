"""Element-wise conformance of the small operators of the denoise step and of the motion VAE against the fp64 references and derived bounds of
tests/smallops_ref.py: csrc/elem.hip's fp32 small projections (gvf_dit_timestep_embed_f32, gvf_dit_modulation_f32, gvf_dit_input_layer_f32,
gvf_dit_final_layer_f32), gvf_dit_timestep_embed_bf16 and gvf_split3_bf16, csrc/vae.hip's gvf_vae_embed and gvf_geglu.

Every case: inputs from a seeded CPU generator; NaN in every padding or gap the contract allows to be unread (ld gaps, mod_ld gaps, rows past
M, guard rows after pos and after the weights, the weights' padding columns); the output inside a sentinel-filled buffer with guard rows before
and after and guard columns where ld > cols, asserted untouched; a second launch giving the same bits; no element outside the bound, none
exempt; the worst |err| / bound printed.  The matrix is smallops_ref's (every listed value of every axis, the named combinations); the shape
conditions that select both final_layer instantiations, the three grid wraps and both vae_embed kernels are asserted where they run.  Every
GVF_EINVAL condition of the eight entry points is tried once with the output asserted untouched."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

import smallops_ref as S
from gvfdiffusion_amd import _lib
from gvfdiffusion_amd.ops import dit_ops, vae_ops          # noqa: F401  (they register the entry points' signatures)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [torch.bfloat16, torch.float16]
GUARD = 3
SENT16, SENT32 = 0x7E5A, 0x7E5A7E5A
NAN = float("nan")
F32 = torch.float32


def _ids(cases):
    return ["-".join(str(v) for v in c) for c in cases]


def _p(t, off=0):
    return None if t is None else ctypes.c_void_p(t.data_ptr() + off)


def _st(dev):
    return _lib.current_stream(dev)


class Out:
    """rows x cols of `dtype` inside a sentinel-filled (rows + 2 GUARD) x ld buffer."""

    def __init__(self, rows, cols, dtype, dev, ld=None):
        self.rows, self.cols, self.ld = rows, cols, ld or cols
        self.it, self.sent = (torch.int32, SENT32) if dtype == F32 else (torch.int16, SENT16)
        self.buf = torch.full((rows + 2 * GUARD, self.ld), self.sent, dtype=self.it, device=dev).view(dtype)
        self.view = self.buf[GUARD:GUARD + rows]

    def untouched(self):
        torch.cuda.synchronize()
        return bool((self.buf.view(self.it) == self.sent).all())

    def run(self, launch, written_cols=None):
        """launch twice: guards intact, same bits; -> the rows x (written_cols or cols) result on the CPU."""
        wc = written_cols or self.cols
        launch()
        torch.cuda.synchronize()
        first = self.buf.view(self.it).clone()
        guard = torch.ones_like(first, dtype=torch.bool)
        guard[GUARD:GUARD + self.rows, :wc] = False
        assert bool((first[guard] == self.sent).all()), "a store outside the rows / columns of the call"
        launch()
        torch.cuda.synchronize()
        assert torch.equal(self.buf.view(self.it), first), "a second launch gave other bits"
        return self.view[:, :wc].cpu()


def padded(t, dev, extra_rows=2, ld=None, fill=NAN):
    """t (rows, cols) on the device inside a NaN-filled (rows + extra_rows) x ld buffer; -> the (rows, cols) view."""
    rows, cols = t.shape
    buf = torch.full((rows + extra_rows, ld or cols), fill, dtype=t.dtype, device=dev)
    buf[:rows, :cols] = t.to(dev)
    return buf[:rows, :cols]


def vec(t, dev):
    return None if t is None else t.to(dev).contiguous()


def check(out, ref, bnd, what, rows=None):
    assert torch.isfinite(ref).all() and torch.isfinite(bnd).all(), "a case whose reference or bound is not finite checks nothing"
    n_bad, worst = S.excess(out, ref, bnd)
    print(f"{what}: worst |err| / bound {worst:.3f}")
    assert n_bad == 0, f"{what}: {n_bad} of {ref.numel()} elements outside the bound (worst {worst:.3g} x)"
    return worst


# ---- final_layer ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", S.FINAL_CASES, ids=_ids(S.FINAL_CASES))
def test_final_layer_elementwise(cuda, case):
    C, Cout, M, rpg, mod, bias, adv = case
    if (C, Cout) == (512, 32):
        assert Cout > 16 and 32 * C * 4 == 65536, "final_layer_f32_kernel<32> with exactly 64 KiB of LDS"
    if M > 4096:
        assert (M + 3) // 4 > 1024, "the 1024-workgroup grid wraps and the prefetch of the next row is live"
    d = S.make_final(*case)
    x = padded(d["x"], cuda, 3)
    w = padded(d["w"], cuda, 2)
    md = None if d["mod"] is None else d["mod"].to(cuda)
    shift, scale = (None, None) if md is None else (md[:, d["shift_off"]:], md[:, d["scale_off"]:])
    b = vec(d["bias"], cuda)
    o = Out(M, Cout, F32, cuda)
    rc = []
    launch = lambda: rc.append(_lib.lib().gvf_dit_final_layer_f32(_p(x), M, C, 1e-6, _p(shift), _p(scale), d.get("mod_ld", 0), rpg if md is not None else 0, _p(w), _p(b), Cout,
                                                                  _p(o.view), _st(cuda)))
    out = o.run(launch)
    assert rc == [0, 0], f"gvf_dit_final_layer_f32 returned {rc}"
    ref, bnd = S.final_layer(d["x"], d["w"], d["bias"], d["shift"], d["scale"], rpg, 1e-6)
    check(out, ref, bnd, f"final_layer {case}")


# ---- input_layer ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", S.INPUT_CASES, ids=_ids(S.INPUT_CASES))
def test_input_layer_elementwise(cuda, case):
    C, Cin, M, pos, bias = case
    d = S.make_input(*case)
    x = padded(d["x"], cuda, 2)
    wt = padded(d["w_t"], cuda, 2)
    ps = None if d["pos"] is None else padded(d["pos"], cuda, 3)
    b = vec(d["bias"], cuda)
    o = Out(M, C, F32, cuda)
    rc = []
    launch = lambda: rc.append(_lib.lib().gvf_dit_input_layer_f32(_p(x), M, Cin, _p(wt), _p(b), _p(ps), d["period"], d["rpg"], C, _p(o.view), _st(cuda)))
    out = o.run(launch)
    assert rc == [0, 0]
    ref, bnd = S.input_layer(d["x"], d["w_t"], d["bias"], d["pos"], d["period"], d["rpg"])
    check(out, ref, bnd, f"input_layer {case}")


# ---- modulation ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", S.MODULATION_CASES, ids=_ids(S.MODULATION_CASES))
def test_modulation_elementwise(cuda, case):
    C, N, B, bias = case
    if N > 65536:
        assert (N + 31) // 32 > 2048, "the 2048-workgroup grid wraps"
    d = S.make_modulation(*case)
    s = padded(d["s"], cuda, 1)
    w = padded(d["w"], cuda, 2)
    b = vec(d["bias"], cuda)
    o = Out(B, N, F32, cuda)
    rc = []
    launch = lambda: rc.append(_lib.lib().gvf_dit_modulation_f32(_p(s), B, C, _p(w), _p(b), N, _p(o.view), _st(cuda)))
    out = o.run(launch)
    assert rc == [0, 0]
    ref, bnd = S.modulation(d["s"], d["w"], d["bias"])
    check(out, ref, bnd, f"modulation {case}")


# ---- timestep embedder ---------------------------------------------------------------------------------------------------------------------

def _run_timestep_f32(cuda, d):
    B, C, F = d["t"].numel(), d["C"], d["F"]
    t = d["t"].to(cuda)
    w0, w2 = padded(d["w0"], cuda, 2), padded(d["w2"], cuda, 2)
    b0, b2 = vec(d["b0"], cuda), vec(d["b2"], cuda)
    o = Out(B, C, F32, cuda)
    te = Out(B, C, F32, cuda) if d["want_t_emb"] else None
    rc = []
    launch = lambda: rc.append(_lib.lib().gvf_dit_timestep_embed_f32(_p(t), B, F, 10000.0, _p(w0), _p(b0), _p(w2), _p(b2), C, _p(o.view), None if te is None else _p(te.view), _st(cuda)))
    out = o.run(launch)
    assert rc == [0, 0]
    if te is None:
        return None, out
    assert torch.equal(te.buf[:GUARD].view(torch.int32), torch.full_like(te.buf[:GUARD].view(torch.int32), SENT32)) and \
        torch.equal(te.buf[GUARD + B:].view(torch.int32), torch.full_like(te.buf[GUARD + B:].view(torch.int32), SENT32)), "t_emb's guard rows"
    return te.view.cpu(), out


@pytest.mark.parametrize("case", S.TIMESTEP_F32_CASES, ids=_ids(S.TIMESTEP_F32_CASES))
def test_timestep_embed_f32_elementwise(cuda, case):
    """The chain against its propagated bound; silu(t_emb) from the kernel's own t_emb; each Linear on its own through the two probes."""
    d = S.make_timestep(*case)
    (te, e_te), (out, e_out) = S.timestep_embed_f32(d["t"], d["F"], d["w0"], d["b0"], d["w2"], d["b2"])
    te_k, out_k = _run_timestep_f32(cuda, d)
    check(out_k, out, e_out, f"timestep_embed_f32 {case} out")
    if te_k is not None:
        check(te_k, te, e_te, f"timestep_embed_f32 {case} t_emb")
        check(out_k, *S.silu(te_k.double(), torch.zeros_like(te)), f"timestep_embed_f32 {case} out from its own t_emb")
    for kind in ("first", "second"):
        p = S.timestep_probe(d, kind)
        (te, e_te), _ = S.timestep_embed_f32(p["t"], p["F"], p["w0"], p["b0"], p["w2"], p["b2"])
        check(_run_timestep_f32(cuda, p)[0], te, e_te, f"timestep_embed_f32 {case} probe {kind}")


def _run_timestep_bf16(cuda, d, ld_pad):
    B, C, F = d["t"].numel(), d["C"], d["F"]
    t = d["t"].to(cuda)
    ldw0, ldw2, ld_out = ((F + 3) & ~3) + 4 * ld_pad, ((C + 3) & ~3) + 8 * ld_pad, C + 5 * ld_pad
    w0, w2 = padded(d["w0"], cuda, 2, ldw0), padded(d["w2"], cuda, 2, ldw2)        # NaN in the padding columns and after the last row
    b0, b2 = vec(d["b0"], cuda), vec(d["b2"], cuda)
    o = Out(B, C, torch.bfloat16, cuda, ld=ld_out)
    te = Out(B, C, F32, cuda) if d["want_t_emb"] else None
    rc = []
    launch = lambda: rc.append(_lib.lib().gvf_dit_timestep_embed_bf16(_p(t), B, F, 10000.0, _p(w0), ldw0, _p(b0), _p(w2), ldw2, _p(b2), C, _p(o.view), ld_out,
                                                                      None if te is None else _p(te.view), _st(cuda)))
    full = o.run(launch, written_cols=ld_out)
    assert rc == [0, 0]
    assert bool((full[:, C:].view(torch.int16) == 0).all()), "the output's padding columns are not +0"
    if te is not None:
        assert bool((te.buf[:GUARD].view(torch.int32) == SENT32).all()) and bool((te.buf[GUARD + B:].view(torch.int32) == SENT32).all())
    return None if te is None else te.view.cpu(), full[:, :C]


@pytest.mark.parametrize("ld_pad", [0, 1], ids=["tight", "padded"])
@pytest.mark.parametrize("case", S.TIMESTEP_BF16_CASES, ids=_ids(S.TIMESTEP_BF16_CASES))
def test_timestep_embed_bf16_elementwise(cuda, case, ld_pad):
    """As the fp32 form, with the operands rounded where the kernel rounds them.  freq_dim % 4 == 2 and C % 4 != 0 leave padding columns in the
    last group of four of every weight row: they hold NaN here (include/gvf_dit.h: loaded but masked)."""
    d = S.make_timestep(*case, dt=torch.bfloat16)
    (te, e_te), (out, e_out) = S.timestep_embed_bf16(d["t"], d["F"], d["w0"], d["b0"], d["w2"], d["b2"])
    te_k, out_k = _run_timestep_bf16(cuda, d, ld_pad)
    check(out_k, out, e_out, f"timestep_embed_bf16 {case} out")
    if te_k is not None:
        check(te_k, te, e_te, f"timestep_embed_bf16 {case} t_emb")
        g, e = S.silu(te_k.double(), torch.zeros_like(te))
        check(out_k, g, S._round_bound(g, e, torch.bfloat16), f"timestep_embed_bf16 {case} out from its own t_emb")
    for kind in ("first", "second"):
        p = S.timestep_probe(d, kind)
        (te, e_te), _ = S.timestep_embed_bf16(p["t"], p["F"], p["w0"], p["b0"], p["w2"], p["b2"])
        check(_run_timestep_bf16(cuda, p, ld_pad)[0], te, e_te, f"timestep_embed_bf16 {case} probe {kind}")


# ---- split3 --------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", S.SPLIT3_CASES, ids=_ids(S.SPLIT3_CASES))
def test_split3_is_exact(cuda, case):
    """hi / lo bit for bit, the layout of the mode, +0 in the padding; an odd ld_src takes the scalar path in most rows, a 16-byte-aligned one the
    vector path; 131100 rows of 32 threads wrap the 16384-workgroup grid."""
    cols, rows, gap, mode = case
    Kp = S.pad64(cols)
    if rows > 100000:
        assert rows * (Kp // 4) > 16384 * 256, "the 16384-workgroup grid wraps"
    ld_src = cols + gap
    x = S.make_split3(cols, rows)
    src = padded(x, cuda, 1, ld_src)
    if gap == 0 and cols % 4 == 0:
        assert src.data_ptr() % 16 == 0 and (ld_src * 4) % 16 == 0, "the vector path"
    o = Out(rows, 3 * Kp, torch.bfloat16, cuda)
    rc = []
    launch = lambda: rc.append(_lib.lib().gvf_split3_bf16(_p(src), ld_src, _p(o.view), rows, cols, mode, _st(cuda)))
    out = o.run(launch)
    assert rc == [0, 0]
    ref = S.split3(x, mode)
    same = out.view(torch.int16) == ref.view(torch.int16)
    assert bool(same.all()), f"{int((~same).sum())} of {same.numel()} values differ from hi = R_bf16(x), lo = R_bf16(x - hi) in the layout of mode {mode}"


# ---- vae_embed -----------------------------------------------------------------------------------------------------------------------------

def _run_vae(cuda, d, dt, want_embed):
    P, C, qdim = d["P"], d["C"], d["qdim"]
    q = padded(d["q"], cuda, 2)
    W = padded(d["W"], cuda, 1)
    b, om = padded(d["b"][None], cuda, 1)[0], padded(d["omega"][None], cuda, 1)[0]
    o = Out(P, C, dt, cuda)
    e = Out(P, C, F32, cuda) if want_embed else None
    rc = []
    launch = lambda: rc.append(_lib.lib().gvf_vae_embed(dit_ops.dt_code(dt), _p(q), qdim, _p(W), _p(b), _p(om), _p(o.view), None if e is None else _p(e.view), P, C,
                                                        d["eps_embed"], d["eps_prenorm"], _st(cuda)))
    out = o.run(launch)
    assert rc == [0, 0], f"gvf_vae_embed returned {rc}"
    emb = None
    if e is not None:
        bits = e.buf.view(torch.int32)
        assert bool((bits[:GUARD] == SENT32).all()) and bool((bits[GUARD + P:] == SENT32).all()), "the embedding's guard rows"
        emb = e.view.cpu()
    return emb, out


def _check_vae(d, dt, emb, out, what):
    (s, e_s), (y, e_y), amb = S.vae_embed(d["q"], d["W"], d["b"], d["omega"], d["eps_embed"], d["eps_prenorm"], dt)
    if emb is not None:
        check(emb, s, e_s, what + " embedding")
    check(out, y, e_y, what + f" out (ambiguous {100 * float((amb > 0).double().mean()):.2f} %)")


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("case", S.VAE_CASES, ids=_ids(S.VAE_CASES))
def test_vae_embed_elementwise(cuda, case, dt):
    C, qdim, P, kind, want_embed = case
    reg = C == 768 and qdim == 14 and os.environ.get("GVF_VAE_EMBED_REG", "1") != "0"
    lds = (C * (qdim | 1) + C + C // 6) * 4
    assert reg or lds <= 65536
    print(f"vae_embed {case}: {'register kernel' if reg else f'LDS kernel, {lds} B'}")
    d = S.make_vae(C, qdim, P, kind)
    emb, out = _run_vae(cuda, d, dt, want_embed)
    _check_vae(d, dt, emb, out, f"vae_embed {case} {dt}")


CHILD = """
import sys, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + '/tests')
import smallops_ref as S, test_smallops_conformance_gpu as T
dev = torch.device('cuda:0')
res = {}
for name, dt in (('bf16', torch.bfloat16), ('fp16', torch.float16)):
    emb, out = T._run_vae(dev, S.make_vae(768, 14, 1000, 'plain'), dt, True)
    res[name] = (emb, out.view(torch.int16))
torch.save(res, sys.argv[2])
"""


def test_vae_embed_register_and_lds_kernel_on_the_same_inputs(cuda, tmp_path):
    """768 x 14: the register kernel here, the LDS kernel in one fresh child process (the switch is read once per process), both inside the band."""
    assert os.environ.get("GVF_VAE_EMBED_REG", "1") != "0"
    d = S.make_vae(768, 14, 1000, "plain")
    path = str(tmp_path / "lds.pt")
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, path], cwd=ROOT, env=dict(os.environ, GVF_VAE_EMBED_REG="0"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lds = torch.load(path)
    for name, dt in (("bf16", torch.bfloat16), ("fp16", torch.float16)):
        emb, out = _run_vae(cuda, d, dt, True)
        _check_vae(d, dt, emb, out, f"vae_embed 768 x 14 register kernel {name}")
        _check_vae(d, dt, lds[name][0], lds[name][1].view(dt), f"vae_embed 768 x 14 LDS kernel {name}")


# ---- geglu ---------------------------------------------------------------------------------------------------------------------------------

def _run_geglu(cuda, x, ld_in_gap, ld_out_gap):
    rows, F = x.shape[0], x.shape[1] // 2
    dt = x.dtype
    src = torch.full((rows + 1, 2 * F + ld_in_gap), NAN, dtype=dt, device=cuda)
    src[:rows, :2 * F] = x.to(cuda)
    o = Out(rows, F, dt, cuda, ld=F + ld_out_gap)
    rc = []
    launch = lambda: rc.append(_lib.lib().gvf_geglu(dit_ops.dt_code(dt), _p(src), 2 * F + ld_in_gap, _p(o.view), F + ld_out_gap, rows, F, _st(cuda)))
    out = o.run(launch)
    assert rc == [0, 0]
    return out


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("case", S.GEGLU_CASES, ids=_ids(S.GEGLU_CASES))
def test_geglu_elementwise(cuda, case, dt):
    F, rows, gi, go = case
    if rows > 10000:
        assert rows * (F // 8) > 16384 * 256, "the 16384-workgroup grid wraps"
    x = S.make_geglu(F, rows, dt)
    out = _run_geglu(cuda, x, gi, go)
    n_bad, worst = 0, 0.0
    for r0 in range(0, rows, 1024):                               # the fp64 reference in slices of 1024 rows
        n, w = S.geglu_check(out[r0:r0 + 1024], x[r0:r0 + 1024])
        n_bad, worst = n_bad + n, max(worst, w)
    print(f"geglu {case} {dt}: worst |err| / bound {worst:.3f}")
    assert n_bad == 0, f"{n_bad} of {rows * F} elements outside their interval"


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
def test_geglu_every_gate_bit_pattern(cuda, dt):
    """Each of the 65 536 gate patterns with every value of GEGLU_VALUES: finite pairs inside the band, the others equal to the fp64 expression
    (NaN for NaN, signed infinities)."""
    x = S.make_geglu_all_gates(dt)
    out = _run_geglu(cuda, x, 0, 0)
    n_bad, worst = S.geglu_check(out, x)
    print(f"geglu every gate {dt}: worst |err| / bound {worst:.3f}")
    assert n_bad == 0, f"{n_bad} of {out.numel()} elements outside their interval"


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------

def _refuse(fn, base, bad, outs):
    """Each (index, value) of `bad` replaces one argument of the valid call `base`: GVF_EINVAL, and nothing written."""
    f = getattr(_lib.lib(), fn)
    for what, changes in bad:
        args = list(base)
        for i, v in changes:
            args[i] = v
        rc = f(*args)
        assert rc == _lib.GVF_EINVAL, f"{fn} with {what}: returned {rc}"
    for o in outs:
        assert o.untouched(), f"{fn}: a refused call wrote to the output"
    rc = f(*base)                                                  # the base call itself is valid
    torch.cuda.synchronize()
    assert rc == 0, f"{fn}: the valid call returned {rc}"


def test_refusals_of_the_small_projections(cuda):
    st = _st(cuda)
    z = lambda *s: torch.zeros(s, device=cuda)
    # final_layer: x, M, C, eps, shift, scale, mod_ld, rpg, w, bias, Cout, out, stream
    x, w, md, o = z(8, 64), z(5, 64), z(2, 136), Out(8, 5, F32, cuda)
    base = [_p(x), 8, 64, 1e-6, _p(md), _p(md, 4 * 68), 136, 4, _p(w), None, 5, _p(o.view), st]
    _refuse("gvf_dit_final_layer_f32", base, [
        ("M < 0", [(1, -1)]), ("C = 0", [(2, 0)]), ("C > 512", [(2, 516)]), ("C % 4", [(2, 62)]), ("Cout = 0", [(10, 0)]), ("Cout > 32", [(10, 33)]),
        ("x null", [(0, None)]), ("w null", [(8, None)]), ("out null", [(11, None)]), ("shift without scale", [(5, None)]), ("scale without shift", [(4, None)]),
        ("x misaligned", [(0, _p(x, 4))]), ("w misaligned", [(8, _p(w, 8))]), ("rows_per_group = 0", [(7, 0)]), ("mod_ld % 4", [(6, 138)]),
        ("scale misaligned", [(5, _p(md, 4 * 69))]), ("shift misaligned", [(4, _p(md, 4))])], [o])
    # input_layer: x, M, Cin, w_t, bias, pos, period, rpg, C, out, stream
    x, wt, pos, o = z(8, 7), z(7, 64), z(4, 64), Out(8, 64, F32, cuda)
    base = [_p(x), 8, 7, _p(wt), None, _p(pos), 2, 4, 64, _p(o.view), st]
    _refuse("gvf_dit_input_layer_f32", base, [
        ("M < 0", [(1, -1)]), ("Cin = 0", [(2, 0)]), ("Cin > 24", [(2, 25)]), ("C = 0", [(8, 0)]), ("C > 512", [(8, 513)]), ("x null", [(0, None)]), ("w null", [(3, None)]),
        ("out null", [(9, None)]), ("pos_period = 0", [(6, 0)]), ("rows_per_group = 0", [(7, 0)]), ("rows_per_group % pos_period", [(6, 3)])], [o])
    # modulation: s, B, C, w, bias, N, out, stream
    s, w, o = z(2, 64), z(9, 64), Out(2, 9, F32, cuda)
    base = [_p(s), 2, 64, _p(w), None, 9, _p(o.view), st]
    _refuse("gvf_dit_modulation_f32", base, [
        ("B < 0", [(1, -1)]), ("C = 0", [(2, 0)]), ("C % 4", [(2, 62)]), ("C > 1024", [(2, 1028)]), ("N = 0", [(5, 0)]), ("s null", [(0, None)]), ("w null", [(3, None)]),
        ("out null", [(6, None)]), ("w misaligned", [(3, _p(w, 4))])], [o])
    # timestep_embed_f32: t, B, F, max_period, w0, b0, w2, b2, C, out, t_emb, stream
    t, w0, w2, o, te = z(2), z(64, 64), z(64, 64), Out(2, 64, F32, cuda), Out(2, 64, F32, cuda)
    base = [_p(t), 2, 64, 10000.0, _p(w0), None, _p(w2), None, 64, _p(o.view), _p(te.view), st]
    _refuse("gvf_dit_timestep_embed_f32", base, [
        ("B < 0", [(1, -1)]), ("freq_dim = 0", [(2, 0)]), ("freq_dim % 4", [(2, 62)]), ("freq_dim > 1024", [(2, 1028)]), ("C = 0", [(8, 0)]), ("C % 4", [(8, 62)]),
        ("C > 1024", [(8, 1028)]), ("max_period = 1", [(3, 1.0)]), ("max_period NaN", [(3, NAN)]), ("t null", [(0, None)]), ("w0 null", [(4, None)]), ("w2 null", [(6, None)]),
        ("out null", [(9, None)]), ("w0 misaligned", [(4, _p(w0, 4))]), ("w2 misaligned", [(6, _p(w2, 8))])], [o, te])
    # timestep_embed_bf16: t, B, F, max_period, w0, ldw0, b0, w2, ldw2, b2, C, out, ld_out, t_emb, stream
    w0, w2 = torch.zeros((62, 64), dtype=torch.bfloat16, device=cuda), torch.zeros((62, 64), dtype=torch.bfloat16, device=cuda)
    o, te = Out(2, 64, torch.bfloat16, cuda), Out(2, 62, F32, cuda)
    base = [_p(t), 2, 62, 10000.0, _p(w0), 64, None, _p(w2), 64, None, 62, _p(o.view), 64, _p(te.view), st]
    _refuse("gvf_dit_timestep_embed_bf16", base, [
        ("B < 0", [(1, -1)]), ("freq_dim = 0", [(2, 0)]), ("freq_dim odd", [(2, 61)]), ("freq_dim > 1024", [(2, 1026)]), ("C = 0", [(10, 0)]), ("C > 1024", [(10, 1025)]),
        ("ldw0 < freq_dim rounded up to 4", [(5, 60)]), ("ldw2 < C rounded up to 4", [(8, 60)]), ("ldw0 % 4", [(5, 66)]), ("ldw2 % 4", [(8, 66)]), ("ld_out < C", [(12, 61)]),
        ("max_period = 1", [(3, 1.0)]), ("t null", [(0, None)]), ("w0 null", [(4, None)]), ("w2 null", [(7, None)]), ("out null", [(11, None)]),
        ("w0 misaligned", [(4, _p(w0, 2))]), ("w2 misaligned", [(7, _p(w2, 4))])], [o, te])


def test_refusals_of_split3_geglu_and_vae_embed(cuda):
    st = _st(cuda)
    z = lambda *s, dt=F32: torch.zeros(s, dtype=dt, device=cuda)
    # split3: src, ld_src, dst, rows, cols, mode, stream
    src, o = z(4, 70), Out(4, 3 * 128, torch.bfloat16, cuda)
    base = [_p(src), 70, _p(o.view), 4, 65, 0, st]
    _refuse("gvf_split3_bf16", base, [("rows < 0", [(3, -1)]), ("cols = 0", [(4, 0)]), ("ld_src < cols", [(1, 64)]), ("mode 2", [(5, 2)]), ("mode -1", [(5, -1)]),
                                      ("src null", [(0, None)]), ("dst null", [(2, None)]), ("dst misaligned", [(2, _p(o.view, 2))])], [o])
    # geglu: dtype, in, ld_in, out, ld_out, rows, F, stream
    x, o = z(4, 32, dt=torch.bfloat16), Out(4, 16, torch.bfloat16, cuda)
    base = [0, _p(x), 32, _p(o.view), 16, 4, 16, st]
    _refuse("gvf_geglu", base, [("dtype 2", [(0, 2)]), ("rows < 0", [(5, -1)]), ("F = 0", [(6, 0)]), ("F % 8", [(6, 12)]), ("ld_in % 8", [(2, 36)]), ("ld_out % 8", [(4, 20)]),
                                ("ld_in < 2 F", [(2, 24)]), ("ld_out < F", [(4, 8)]), ("in null", [(1, None)]), ("out null", [(3, None)]), ("in misaligned", [(1, _p(x, 8))]),
                                ("out misaligned", [(3, _p(o.view, 8))])], [o])
    # vae_embed: dtype, q, qdim, W, bias, omega, out16, out_embed, P, C, eps_embed, eps_prenorm, stream
    q, W, b, om = z(4, 16), z(1020, 16), z(1020), z(170)
    o, e = Out(4, 1020, torch.bfloat16, cuda), Out(4, 1020, F32, cuda)
    base = [0, _p(q), 14, _p(W), _p(b), _p(om), _p(o.view), _p(e.view), 4, 96, 1e-5, 1e-6, st]
    assert (1020 * 15 + 1020 + 170) * 4 == 65960 and (1008 * 15 + 1008 + 168) * 4 <= 65536 and (906 * 17 + 906 + 151) * 4 > 65536 and (900 * 17 + 900 + 150) * 4 <= 65536
    _refuse("gvf_vae_embed", base, [("dtype 2", [(0, 2)]), ("P < 0", [(8, -1)]), ("qdim < 3", [(2, 2)]), ("qdim > 16", [(2, 17)]), ("C = 0", [(9, 0)]), ("C > 1024", [(9, 1026)]),
                                    ("C % 6", [(9, 100)]), ("65 960 B of LDS (C = 1020, qdim = 14)", [(9, 1020)]), ("over 64 KiB of LDS (C = 906, qdim = 16)", [(9, 906), (2, 16)]),
                                    ("queries null", [(1, None)]), ("W null", [(3, None)]), ("bias null", [(4, None)]), ("omega null", [(5, None)]), ("out null", [(6, None)])], [o, e])
    for C, qdim in ((1008, 14), (900, 16)):                       # the largest accepted widths launch
        d = S.make_vae(C, qdim, 65, "plain")
        emb, out = _run_vae(cuda, d, torch.bfloat16, True)
        _check_vae(d, torch.bfloat16, emb, out, f"vae_embed {C} x {qdim} (the LDS limit)")
