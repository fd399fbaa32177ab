"""The motion-VAE training kernels (csrc/vae_train.hip) against the float64 formulas of tests/vae_train_ref.py on the same inputs, with the
harness and the convention of tests/test_sparse_train_ops_gpu.py: every tensor output by relative L2 over the whole tensor and over its worst
block of 32 rows, the bar being TWICE the error of the fp32 torch yardstick (the same formulas as a naive fp32 composition with the kernels'
rounding points).  The per-group KL terms and the KL part of the gradient are held to DERIVED bounds instead (vae_train_ref.kl_groups_bound /
dkl_bound).  Also: NaN bands and NaN padding columns around every result stay NaN, the workspace starts as NaN, the same bits on a second launch
and on another stream.  The entry points are called through ctypes on buffers of the test's own."""
import pytest
import torch

import vae_train_ref as R
from gvfdiffusion_amd import _lib
from gvfdiffusion_amd.ops import dit_ops, vae_train as V
from test_dit_train_ops_gpu import _check, _p, _stream_ptr, _twice_and_other_stream
from test_sparse_train_ops_gpu import _band, _bands_nan, _put, _ws

pytestmark = pytest.mark.gpu
DTYPES = [torch.bfloat16, torch.float16]
NAN = float("nan")


def _padded(t, ld):
    """t [rows, w] inside a [rows, ld] matrix whose other columns are NaN"""
    wide = torch.full((t.shape[0], ld), NAN, dtype=t.dtype)
    wide[:, :t.shape[1]] = t
    return wide


# ---- GEGLU ------------------------------------------------------------------------------------------------------------------------------
def _geglu_launch(dt, u, da, F_, cuda):
    """u [rows, 2F], da [rows, F] on the host -> (a, du) from the device, through row strides larger than the rows, with every check on bands,
    padding and repeatability"""
    rows = u.shape[0]
    ldu, lda, ldda, lddu = 2 * F_ + 16, F_ + 8, F_ + 24, 2 * F_ + 8
    ub, ud = _put(_padded(u, ldu), cuda)
    gb, gd = _put(_padded(da, ldda), cuda)
    ab, a = _band((rows, lda), dt, cuda)
    db, du = _band((rows, lddu), dt, cuda)
    code = dit_ops.dt_code(dt)

    def launch(stream):
        sp = _stream_ptr(stream)
        _lib.check(_lib.lib().gvf_geglu_fwd(code, _p(ud), ldu, _p(a), lda, rows, F_, sp), "fwd")
        _lib.check(_lib.lib().gvf_geglu_bwd(code, _p(ud), ldu, _p(gd), ldda, _p(du), lddu, rows, F_, sp), "bwd")
    _twice_and_other_stream(launch, [ab, db])
    for buf, n in ((ub, rows * ldu), (gb, rows * ldda), (ab, rows * lda), (db, rows * lddu)):
        assert _bands_nan(buf, n), "a store outside the rows of the call"
    assert bool(torch.isnan(a[:, F_:].float()).all()) and bool(torch.isnan(du[:, 2 * F_:].float()).all()), "the padding columns were written"
    return a[:, :F_].cpu(), du[:, :2 * F_].cpu()


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("F_", [96, 3072])
@pytest.mark.parametrize("rows", [1, 33, 257])
def test_geglu_forward_and_backward(cuda, dt, rows, F_):
    g = torch.Generator().manual_seed(rows + F_)
    u = (torch.randn((rows, 2 * F_), generator=g) * 3).to(dt)
    da = torch.randn((rows, F_), generator=g).to(dt)
    for i, v in enumerate((0.0, 20.0, -20.0, 14.0, -14.0, 13.9, -6.0, 5.5)):      # 0, saturated, the edge of the dropped term, the tails
        u[i % rows, F_ + 3 * i + 1] = v
    ref, yard = R.geglu(u.float(), da.float()), R.geglu(u.float(), da.float(), dtype=torch.float32, lp=dt)
    a, du = _geglu_launch(dt, u, da, F_, cuda)
    tag, log = f"geglu rows{rows} F{F_} {dt}", []
    _check(tag, "a", a, ref["a"], yard["a"], log)
    _check(tag, "dx", du[:, :F_], ref["du"][:, :F_], yard["du"][:, :F_], log)
    _check(tag, "dg", du[:, F_:], ref["du"][:, F_:], yard["du"][:, F_:], log)
    print(tag, "| kernel/yardstick:", "; ".join(log))


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
def test_geglu_is_finite_over_the_whole_range_of_the_type(cuda, dt):
    """Gates at 0, the type's denormals, the cut-off and +- the largest finite value beside moderate x and da: finite a and du equal to the
    float64 formula to one rounding of the type.  Then EVERY combination of extreme x, g and da (0 and the largest finite value among them):
    where the exact result does not fit the type the output is an infinity, but never a NaN (no inf * 0)."""
    fi = torch.finfo(dt)
    tiny = fi.smallest_normal * fi.eps                                   # the smallest denormal
    gates = [0.0, -0.0, tiny, -tiny, 37 * tiny, fi.smallest_normal / 2, 1.0, 6.0, -6.0, 13.5, -13.5, 14.0, -14.0, 40.0, -40.0, fi.max / 2, -fi.max / 2,
             fi.max, -fi.max]
    xs = [1.0, -0.75, 0.5]                                               # |x|, |da| <= 1: the exact results fit the type at every gate
    F_ = 8 * len(xs)
    u = torch.zeros((len(gates), 2 * F_))
    for i, gv in enumerate(gates):
        u[i, F_:] = gv
        u[i, :F_] = torch.tensor(xs).repeat_interleave(8)
    u = u.to(dt)
    da = torch.full((len(gates), F_), 0.75).to(dt)
    a, du = _geglu_launch(dt, u, da, F_, cuda)
    ref = R.geglu(u.float(), da.float())
    assert torch.isfinite(a.float()).all() and torch.isfinite(du.float()).all()
    for got, want in ((a, ref["a"]), (du, ref["du"])):
        # one rounding of the type (half of eps; eps leaves room for the fp32 arithmetic in front of it), erff's absolute error on Phi beside
        # |x da| <= 1 (1e-6 with room), or one denormal
        assert bool(((got.double() - want).abs() <= fi.eps * want.abs() + 1e-6 + tiny).all())
    big = u.float()[:, F_:].abs() >= 40
    pos = u.float()[:, F_:] > 0
    x = u.float()[:, :F_]
    assert torch.equal(a.float()[big & ~pos].abs(), torch.zeros_like(a.float()[big & ~pos])), "a saturated negative gate gives 0"
    assert torch.equal(du.float()[:, F_:][big & pos], (da.float() * x)[big & pos]) and not bool(du.float()[:, F_:][big & ~pos].any())
    ext = [0.0, fi.max, -fi.max, 1.4, -0.75]
    combos = torch.cartesian_prod(torch.tensor(ext), torch.tensor(ext), torch.tensor(ext))          # (x, g, da)
    n = (combos.shape[0] + 7) // 8 * 8
    c = torch.zeros((n, 3))
    c[:combos.shape[0]] = combos
    u2 = torch.cat([c[:, 0].reshape(-1, 8), c[:, 1].reshape(-1, 8)], dim=1).to(dt)
    da2 = c[:, 2].reshape(-1, 8).to(dt)
    a2, du2 = _geglu_launch(dt, u2, da2, 8, cuda)
    assert not bool(torch.isnan(a2.float()).any()) and not bool(torch.isnan(du2.float()).any()), "inf * 0 somewhere"


def test_geglu_autograd(cuda):
    g = torch.Generator().manual_seed(4)
    wide = torch.randn((33, 2 * 96 + 16), generator=g).to(torch.bfloat16).to(cuda).requires_grad_()
    w = torch.randn((33, 96), generator=g).to(torch.bfloat16).to(cuda)
    a = V.geglu(wide[:, 8:8 + 192])                                      # a column slice: read through its stride
    (a.float() * w.float()).sum().backward()
    ref = R.geglu(wide.detach()[:, 8:200].float().cpu(), w.float().cpu())
    assert R.rel_l2(a.detach().cpu(), ref["a"]) <= 2.0 ** -8 and R.rel_l2(wide.grad[:, 8:200].cpu(), ref["du"]) <= 2.0 ** -8
    assert float(wide.grad[:, :8].abs().max()) == 0 and float(wide.grad[:, 200:].abs().max()) == 0
    a3 = V.geglu(wide.detach()[:, 8:200].reshape(3, 11, 192))
    assert a3.shape == (3, 11, 96) and torch.equal(a3.reshape(33, 96), a.detach())
    with pytest.raises(ValueError):
        V.geglu(wide[:, :24])


# ---- embedding --------------------------------------------------------------------------------------------------------------------------
def _embed_inputs(P, qdim, C, seed):
    g = torch.Generator().manual_seed(seed)
    r = torch.randn((P, qdim), generator=g) * 0.5
    r[:, :3] = torch.rand((P, 3), generator=g) - 0.5                      # xyz in the unit cube
    W = torch.randn((C, qdim), generator=g) * 0.3
    if qdim == 6:
        W[:, :3] = 0.0                                                   # the encoder's input_embedding: zero columns on the xyz part
    b = torch.randn(C, generator=g) * 0.1
    E = C // 6
    omega = (1.0 / 10000 ** (torch.arange(E, dtype=torch.float64) / (E / 2.0))).float()
    de = torch.randn((P, C), generator=g)
    return r, W, b, omega, de


@pytest.mark.parametrize("want_dr", [True, False], ids=["dr", "nodr"])
@pytest.mark.parametrize("qdim,C", [(6, 192), (14, 192), (14, 768)])
@pytest.mark.parametrize("P", [1, 63, 4099])
def test_embed_forward_and_backward(cuda, P, qdim, C, want_dr):
    """P = 4099: 342 workgroups' partials of dW and db go through the finaliser (63: 16, 1: one)"""
    r, W, b, omega, de = _embed_inputs(P, qdim, C, P * 5 + qdim + C)
    ref, yard = R.embed(r, W, b, omega, de), R.embed(r, W, b, omega, de, dtype=torch.float32)
    rb, rd = _put(r, cuda)
    wb, wd = _put(W, cuda)
    bb, bd = _put(b, cuda)
    ob, od = _put(omega, cuda)
    gb, gd = _put(de, cuda)
    eb, e = _band((P, C), torch.float32, cuda)
    dwb, dW = _band((C, qdim), torch.float32, cuda)
    dbb, db = _band((C,), torch.float32, cuda)
    drb, dr = _band((P, qdim), torch.float32, cuda)
    ws = _ws("gvf_vae_embed_bwd_workspace_bytes", cuda, P, qdim, C)

    def launch(stream):
        sp = _stream_ptr(stream)
        _lib.check(_lib.lib().gvf_vae_embed_train_fwd(_p(rd), qdim, _p(wd), _p(bd), _p(od), _p(e), P, C, 1e-5, sp), "fwd")
        _lib.check(_lib.lib().gvf_vae_embed_bwd(_p(rd), qdim, _p(wd), _p(bd), _p(od), _p(gd), _p(dW), _p(db), _p(dr) if want_dr else None, P, C, 1e-5,
                                                _p(ws), ws.numel() * 8, sp), "bwd")
    _twice_and_other_stream(launch, [eb, dwb, dbb, drb])
    for buf, n in ((rb, P * qdim), (wb, C * qdim), (bb, C), (ob, C // 6), (gb, P * C), (eb, P * C), (dwb, C * qdim), (dbb, C), (drb, P * qdim)):
        assert _bands_nan(buf, n), "a store outside the rows of the call"
    tag, log = f"embed P{P} q{qdim} C{C} {'dr' if want_dr else 'nodr'}", []
    _check(tag, "e", e.cpu(), ref["e"], yard["e"], log)
    _check(tag, "dW", dW.cpu(), ref["dW"], yard["dW"], log)
    _check(tag, "db", db.cpu().reshape(-1, 1), ref["db"].reshape(-1, 1), yard["db"].reshape(-1, 1), log)
    if want_dr:
        _check(tag, "dr", dr.cpu(), ref["dr"], yard["dr"], log)
    else:
        assert bool(torch.isnan(dr).all()), "dr was written although no pointer was given"
    print(tag, "| kernel/yardstick:", "; ".join(log))


def test_embed_autograd(cuda):
    r, W, b, omega, de = _embed_inputs(63, 14, 192, 11)
    ref = R.embed(r, W, b, omega, de)
    rl, Wl, bl = r.to(cuda).requires_grad_(), W.to(cuda).requires_grad_(), b.to(cuda).requires_grad_()
    e = V.embed(rl, Wl, bl, omega.to(cuda))
    e.backward(de.to(cuda))
    assert R.rel_l2(e.detach().cpu(), ref["e"]) <= 1e-6 and R.rel_l2(Wl.grad.cpu(), ref["dW"]) <= 1e-5
    assert R.rel_l2(bl.grad.cpu(), ref["db"]) <= 1e-5 and R.rel_l2(rl.grad.cpu(), ref["dr"]) <= 1e-5
    e2 = V.embed(r.to(cuda), Wl, bl, omega.to(cuda))                     # rows without a gradient: dr is not computed
    gW, = torch.autograd.grad(e2, Wl, de.to(cuda))
    assert torch.equal(gW, Wl.grad) and torch.equal(e2, e.detach())
    with pytest.raises(ValueError):
        V.embed(rl, W.to(cuda)[:100], b.to(cuda)[:100], omega.to(cuda))


# ---- grouped posterior ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["slices", "shifted"])
@pytest.mark.parametrize("G,L,Dl", [(1, 1, 16), (6, 40, 16), (3, 513, 8)])
def test_posterior_groups_forward_and_backward(cuda, G, L, Dl, layout):
    """slices: mean and logvar are two column slices of one [rows, 2 Dl + 4] matrix (float4 path); shifted: contiguous tensors 4 bytes off a
    16-byte boundary (the element-wise path).  (3, 513, 8): two workgroups' partials per group."""
    g = torch.Generator().manual_seed(G * 7 + L + Dl)
    rows, n = G * L, L * Dl
    mean = torch.randn((rows, Dl), generator=g) * 2
    logvar = torch.randn((rows, Dl), generator=g) * 1.5 - 1
    for i, v in enumerate((-31.0, -30.0, 20.0, 21.0, -45.0, 33.0, 6.0)):  # outside, exactly on the bounds, and one large variance inside
        logvar[(i * 5) % rows, (i * 3) % Dl] = v
    eps, dz = torch.randn((rows, Dl), generator=g), torch.randn((rows, Dl), generator=g)
    dkl = (torch.rand(G, generator=g) + 0.2) * 0.37 * n                  # so that the KL part of the gradient is the size of the dz part
    ref = R.posterior_groups(mean, logvar, eps, dz, dkl, G)
    yard = R.posterior_groups(mean, logvar, eps, dz, dkl, G, dtype=torch.float32)
    if layout == "slices":
        ld, shift = 2 * Dl + 4, 0
        hb, hd = _put(_padded(torch.cat([mean, logvar], dim=1), ld), cuda)
        md, lvd = hd[:, :Dl], hd[:, Dl:2 * Dl]
        gbuf, gh = _band((rows, ld), torch.float32, cuda)
        dm, dl = gh[:, :Dl], gh[:, Dl:2 * Dl]
    else:
        ld, shift = Dl, 1
        hb, md = _put(mean, cuda, shift)
        lb, lvd = _put(logvar, cuda, shift)
        gbuf, dm = _band((rows, Dl), torch.float32, cuda, shift)
        g2buf, dl = _band((rows, Dl), torch.float32, cuda, shift)
    eb, ed = _put(eps, cuda, shift)
    zb, zd = _put(dz, cuda, shift)
    kb, kd = _put(dkl, cuda)
    ob, z = _band((rows, Dl), torch.float32, cuda, shift)
    klb, kl = _band((G,), torch.float32, cuda)
    ws = _ws("gvf_posterior_groups_workspace_bytes", cuda, G, L, Dl)
    lib = _lib.lib()

    def launch(stream):
        sp = _stream_ptr(stream)
        _lib.check(lib.gvf_posterior_groups_fwd(_p(md), ld, _p(lvd), ld, _p(ed), _p(z), _p(kl), G, L, Dl, _p(ws), ws.numel() * 8, sp), "fwd")
        _lib.check(lib.gvf_posterior_groups_bwd(_p(md), ld, _p(lvd), ld, _p(ed), _p(zd), _p(kd), _p(dm), ld, _p(dl), ld, G, L, Dl, sp), "bwd")
    outs = [ob, klb, gbuf] + ([g2buf] if layout == "shifted" else [])
    _twice_and_other_stream(launch, outs)
    assert _bands_nan(ob, rows * Dl, shift) and _bands_nan(klb, G) and _bands_nan(eb, rows * Dl, shift) and _bands_nan(zb, rows * Dl, shift)
    if layout == "slices":
        assert _bands_nan(gbuf, rows * ld) and _bands_nan(hb, rows * ld)
        assert bool(torch.isnan(gh[:, 2 * Dl:]).all()), "the padding columns of the gradient were written"
    else:
        assert _bands_nan(gbuf, rows * Dl, shift) and _bands_nan(g2buf, rows * Dl, shift)
    tag, log = f"posterior_groups G{G} L{L} Dl{Dl} {layout}", []
    _check(tag, "z", z.cpu(), ref["z"], yard["z"], log)
    _check(tag, "dmean", dm.cpu(), ref["dmean"], yard["dmean"], log)
    _check(tag, "dlogvar", dl.cpu(), ref["dlogvar"], yard["dlogvar"], log)
    outside = (logvar < -30) | (logvar > 20)
    assert bool(outside.any()) and not bool(dl.cpu()[outside].any()), "the clamp blocks the gradient strictly outside its bounds"
    on = (logvar == -30) | (logvar == 20)
    assert bool(on.any()) and bool((dl.cpu()[on] != 0).all()), "the clamp passes the gradient on its bounds"
    err, bound = (kl.cpu().double() - ref["kl"]).abs(), R.kl_groups_bound(mean, logvar, G)
    print(tag, "| kernel/yardstick:", "; ".join(log), f"| kl err/bound max {float((err / bound).max()):.3f} (fp32 torch: "
          f"{float(((yard['kl'].double() - ref['kl']).abs() / bound).max()):.3f})")
    assert bool((err <= bound).all()), f"{tag}: |kl - kl64| = {err.tolist()} > {bound.tolist()}"
    # dz null (and eps with it): the KL part alone, element by element inside its derived bound; dkl null: the sample part alone
    only_kl = torch.empty((2, rows, Dl), device=cuda)
    only_z = torch.empty((2, rows, Dl), device=cuda)
    _lib.check(lib.gvf_posterior_groups_bwd(_p(md), ld, _p(lvd), ld, None, None, _p(kd), _p(only_kl[0]), Dl, _p(only_kl[1]), Dl, G, L, Dl, None), "bwd kl")
    _lib.check(lib.gvf_posterior_groups_bwd(_p(md), ld, _p(lvd), ld, _p(ed), _p(zd), None, _p(only_z[0]), Dl, _p(only_z[1]), Dl, G, L, Dl, None), "bwd z")
    rk = R.posterior_groups(mean, logvar, eps, None, dkl, G)
    bm, bl = R.dkl_bound(mean, logvar, dkl, G)
    inside = (~outside).double()
    assert bool(((only_kl[0].cpu().double() - rk["dmean"]).abs() <= bm).all()), "the KL part of dmean leaves its bound"
    assert bool(((only_kl[1].cpu().double() - rk["dlogvar"]).abs() <= bl * inside).all()), "the KL part of dlogvar leaves its bound"
    parts_m, parts_l = only_kl[0].cpu().double() + only_z[0].cpu().double(), only_kl[1].cpu().double() + only_z[1].cpu().double()
    assert R.rel_l2(parts_m, ref["dmean"]) <= 2 * max(R.rel_l2(yard["dmean"], ref["dmean"]), 2.0 ** -24)
    assert R.rel_l2(parts_l, ref["dlogvar"]) <= 2 * max(R.rel_l2(yard["dlogvar"], ref["dlogvar"]), 2.0 ** -24)


def test_posterior_groups_autograd(cuda):
    g = torch.Generator().manual_seed(9)
    G, L, Dl = 6, 40, 16
    rows = G * L
    wide = torch.randn((rows, 2 * Dl), generator=g).to(cuda).requires_grad_()
    eps = torch.randn((rows, Dl), generator=g).to(cuda)
    w, wk = torch.randn((rows, Dl), generator=g).to(cuda), torch.randn(G, generator=g).to(cuda)
    z, kl = V.posterior_groups(wide[:, :Dl], wide[:, Dl:], eps, G)       # the two halves of one N = 2 Dl projection, read in place
    assert z.shape == (rows, Dl) and kl.shape == (G,)
    ((z * w).sum() + (kl * wk).sum()).backward()
    w64 = wide.detach().double().requires_grad_()
    m, lv = w64[:, :Dl].view(G, L, Dl), torch.clamp(w64[:, Dl:].view(G, L, Dl), -30.0, 20.0)
    z64 = m + torch.exp(0.5 * lv) * eps.double().view(G, L, Dl)
    kl64 = 0.5 * torch.mean(m.pow(2) + lv.exp() - 1.0 - lv, dim=[1, 2])
    ((z64 * w.double().view(G, L, Dl)).sum() + (kl64 * wk.double()).sum()).backward()
    assert R.rel_l2(wide.grad, w64.grad) <= 1e-6 and R.rel_l2(kl, kl64) <= 1e-6
    _, kk = V.posterior_groups(wide[:, :Dl], wide[:, Dl:], eps, G)
    gk, = torch.autograd.grad(kk.mean(), wide)                           # kl alone: z's gradient arrives as None
    assert torch.isfinite(gk).all() and float(gk.abs().max()) > 0
    with pytest.raises(ValueError):
        V.posterior_groups(wide[:, :Dl], wide[:, Dl:], eps, 7)
