"""The static-VAE training kernels (csrc/sparse_train.hip) against the float64 formulas of tests/sparse_train_ref.py on the same inputs, with
the harness and the convention of tests/test_dit_train_ops_gpu.py: every tensor output by relative L2 over the whole tensor and over its worst
block of 32 rows, the bar being TWICE the error of the fp32 yardstick (the same formulas as a naive fp32 composition with the kernels' rounding
points).  Scalars (kl, vol, opa) are held to DERIVED bounds instead (sparse_train_ref.kl_bound / reg_bounds): a scalar yardstick can be exact by
luck.  The gather is bit-exact.  Also: NaN bands around every operand and result stay NaN, the workspace starts as NaN, the same bits on a
second launch and on another stream.  The entry points are called through ctypes on buffers of the test's own."""
import ctypes

import pytest
import torch

import sparse_train_ref as R
from gvfdiffusion_amd import _lib
from gvfdiffusion_amd.ops import dit_ops, sparse_train as S
from test_dit_train_ops_gpu import _check, _p, _stream_ptr, _twice_and_other_stream

pytestmark = pytest.mark.gpu
DTYPES = [torch.bfloat16, torch.float16]
BAND = 64                                       # elements: a multiple of 16 bytes in every type, so the view keeps the buffer's alignment


def _band(shape, dtype, dev, shift=0):
    """(flat buffer of NaN, the view of `shape` inside it, BAND + shift elements from its start)"""
    n = 1
    for s in shape:
        n *= s
    fill = float("nan") if dtype.is_floating_point else -1           # (an index tensor has no NaN; its bands are never read)
    buf = torch.full((n + 2 * BAND + shift,), fill, dtype=dtype, device=dev)
    return buf, buf[BAND + shift:BAND + shift + n].view(shape)


def _put(t, dev, shift=0):
    buf, v = _band(tuple(t.shape), t.dtype, dev, shift)
    v.copy_(t)
    return buf, v


def _bands_nan(buf, n, shift=0):
    return bool(torch.isnan(buf[:BAND + shift].float()).all()) and bool(torch.isnan(buf[BAND + shift + n:].float()).all())


def _ws(name, dev, *dims):
    nb = ctypes.c_size_t(0)
    assert getattr(_lib.lib(), name)(*dims, ctypes.byref(nb)) == _lib.GVF_OK
    return torch.full((int(nb.value) // 8 + 2,), float("nan"), dtype=torch.float64, device=dev)      # NaN: a slot read before it is written shows


# ---- GELU ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("n,shift", [(1, 0), (7, 0), (8, 0), (2047, 0), (2048, 0), (2049, 0), (2049, 1), (300 * 512, 0)])
def test_gelu_forward_and_backward(cuda, dt, n, shift):
    """shift = 1: every pointer 2 bytes off a 16-byte boundary, the element-wise path over the whole tensor"""
    g = torch.Generator().manual_seed(n + shift)
    u = (torch.randn(n, generator=g) * 3).to(dt)
    da = torch.randn(n, generator=g).to(dt)
    for i, v in enumerate((0.0, 20.0, -20.0, 9.0, -9.0, 5.5)):      # 0, +-20 (saturated), the edge of the dropped term, the flat tail
        if 3 * i + 1 < n:
            u[3 * i + 1] = v
    ref, yard = R.gelu(u.float(), da.float()), R.gelu(u.float(), da.float(), dtype=torch.float32, lp=dt)
    ub, ud = _put(u, cuda, shift)
    gb, gd = _put(da, cuda, shift)
    ab, a = _band((n,), dt, cuda, shift)
    db, du = _band((n,), dt, cuda, shift)
    code = dit_ops.dt_code(dt)

    def launch(stream):
        sp = _stream_ptr(stream)
        _lib.check(_lib.lib().gvf_gelu_tanh_fwd(code, _p(ud), _p(a), n, sp), "fwd")
        _lib.check(_lib.lib().gvf_gelu_tanh_bwd(code, _p(ud), _p(gd), _p(du), n, sp), "bwd")
    _twice_and_other_stream(launch, [ab, db])
    for buf in (ub, gb, ab, db):
        assert _bands_nan(buf, n, shift), "a store outside the elements of the call"
    tag, log = f"gelu n{n} shift{shift} {dt}", []
    _check(tag, "a", a.cpu().reshape(-1, 1), ref["a"].reshape(-1, 1), yard["a"].reshape(-1, 1), log)
    _check(tag, "du", du.cpu().reshape(-1, 1), ref["du"].reshape(-1, 1), yard["du"].reshape(-1, 1), log)
    print(tag, "| kernel/yardstick:", "; ".join(log))


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
def test_gelu_is_finite_over_the_whole_range_of_the_type(cuda, dt):
    """0, the type's denormals, +-20 and +- the largest finite value: finite a and du; at +-max exactly u / 0 forward and da / 0 backward (tanh
    saturated, no inf * 0); a denormal u gives 0.5 u to one unit of the type's smallest denormal."""
    fi = torch.finfo(dt)
    tiny = fi.smallest_normal * fi.eps                     # the smallest denormal
    vals = torch.tensor([0.0, -0.0, tiny, -tiny, 37 * tiny, fi.smallest_normal / 2, 20.0, -20.0, fi.max, -fi.max, fi.max / 2, -fi.max / 2, 1.0])
    u = vals.to(dt)
    da = torch.full_like(u, 1.5)
    ub, ud = _put(u, cuda)
    gb, gd = _put(da, cuda)
    n = u.numel()
    ab, a = _band((n,), dt, cuda)
    db, du = _band((n,), dt, cuda)
    code = dit_ops.dt_code(dt)
    _lib.check(_lib.lib().gvf_gelu_tanh_fwd(code, _p(ud), _p(a), n, None), "fwd")
    _lib.check(_lib.lib().gvf_gelu_tanh_bwd(code, _p(ud), _p(gd), _p(du), n, None), "bwd")
    torch.cuda.synchronize()
    a, du = a.cpu().float(), du.cpu().float()
    assert torch.isfinite(a).all() and torch.isfinite(du).all()
    uf = u.float()
    big = uf.abs() >= 20
    assert torch.equal(a[big], torch.where(uf[big] > 0, uf[big], torch.zeros_like(uf[big])))
    assert torch.equal(du[big], torch.where(uf[big] > 0, da.float()[big], torch.zeros_like(uf[big])))
    small = uf.abs() < fi.smallest_normal
    assert bool(((a[small].double() - 0.5 * uf[small].double()).abs() <= tiny).all())
    assert bool(((du[small] - 0.75).abs() <= 0.75 * fi.eps).all())                  # g'(0) = 0.5


# ---- gather -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width_bytes", [16, 48, 384, 4608])
@pytest.mark.parametrize("rows", [1, 5, 257])
def test_gather_rows_is_bit_exact(cuda, rows, width_bytes):
    g = torch.Generator().manual_seed(rows + width_bytes)
    for dt in (torch.float16, torch.bfloat16, torch.float32):
        W = width_bytes // torch.empty((), dtype=dt).element_size()
        src_rows = rows + 3
        x = torch.randn((src_rows, W), generator=g).to(dt)
        wide = torch.full((src_rows, W + 16 // x.element_size() * 2), float("nan"), dtype=dt)       # a strided source: the columns in the middle
        off = 16 // x.element_size()
        wide[:, off:off + W] = x
        perm = torch.randperm(rows, generator=g)
        rep = torch.randint(0, src_rows, (rows,), generator=g)
        for index in (perm, rep):
            for strided in (False, True):
                if strided:
                    sb, sv = _put(wide, cuda)
                    src, stride = sv[:, off:off + W], wide.shape[1] * x.element_size()
                else:
                    sb, src = _put(x, cuda)
                    stride = width_bytes
                ib, idx = _put(index, cuda)
                ob, out = _band((rows, W), dt, cuda)

                def launch(stream):
                    _lib.check(_lib.lib().gvf_gather_rows(_p(src), stride, _p(idx), _p(out), rows, width_bytes, _stream_ptr(stream)), "gather")
                _twice_and_other_stream(launch, [ob])
                assert _bands_nan(ob, rows * W), "a store outside the rows of the call"
                assert torch.equal(out.cpu().view(torch.uint8), x.index_select(0, index).view(torch.uint8))


@pytest.mark.parametrize("dt", [torch.float16, torch.float32])
def test_gather_rows_autograd(cuda, dt):
    """With `inverse` the gradient is the same kernel on the inverse permutation: torch.equal to the gradient of x[idx]; without it (an index
    with repeats) torch's index_add_ -- equal up to the order of its atomic adds, which is exact for an index used at most twice here."""
    g = torch.Generator().manual_seed(5)
    rows, W = 257, 192
    x = torch.randn((rows, W), generator=g).to(dt).to(cuda)
    perm = torch.randperm(rows, generator=g).to(cuda)
    inv = torch.empty_like(perm)
    inv[perm] = torch.arange(rows, device=cuda)
    dy = torch.randn((rows, W), generator=g).to(dt).to(cuda)
    xa, xb = x.clone().requires_grad_(), x.clone().requires_grad_()
    ya, yb = S.gather_rows(xa, perm, inv), xb[perm]
    assert torch.equal(ya, yb)
    ga, = torch.autograd.grad(ya, xa, dy)
    gb, = torch.autograd.grad(yb, xb, dy)
    assert torch.equal(ga, gb)
    # a column slice of a packed matrix is read in place, and its gradient lands in the slice
    packed = torch.randn((rows, 3 * W), generator=g).to(dt).to(cuda).requires_grad_()
    y = S.gather_rows(packed[:, W:2 * W], perm, inv)
    assert torch.equal(y, packed.detach()[:, W:2 * W][perm])
    gp, = torch.autograd.grad(y, packed, dy)
    assert torch.equal(gp[:, W:2 * W], gb) and float(gp[:, :W].abs().max()) == 0 and float(gp[:, 2 * W:].abs().max()) == 0
    rep = torch.cat([torch.arange(rows), torch.arange(0, rows, 2)]).to(cuda)       # every even row twice
    dy2 = torch.randn((rep.numel(), W), generator=g).to(dt).to(cuda)
    xc, xd = x.clone().requires_grad_(), x.clone().requires_grad_()
    gc, = torch.autograd.grad(S.gather_rows(xc, rep), xc, dy2)
    gd, = torch.autograd.grad(xd[rep], xd, dy2)
    assert torch.equal(gc, gd)                                                      # two addends commute
    with pytest.raises(ValueError):
        S.gather_rows(x[:, :3], perm)                                               # rows of 6 / 12 bytes


# ---- posterior ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("strided", [False, True], ids=["contiguous", "strided"])
@pytest.mark.parametrize("L", [8, 3])
@pytest.mark.parametrize("T", [1, 77, 4099])
def test_posterior_forward_and_backward(cuda, T, L, strided):
    g = torch.Generator().manual_seed(T * 3 + L)
    ld = 2 * L + (4 if strided else 0)                           # [mean L | logvar L | 4 NaN]
    h = torch.full((T, ld), float("nan"))
    h[:, :L] = torch.randn((T, L), generator=g) * 2
    h[:, L:2 * L] = torch.randn((T, L), generator=g) * 1.5 - 1
    h[0, L] = 6.0                                                # one large variance: exp(lv) = 403 beside terms of size 1
    eps, dz = torch.randn((T, L), generator=g), torch.randn((T, L), generator=g)
    dkl = 0.37 * T * L                                           # so that the KL part of dh is the size of the dz part
    ref = R.posterior(h[:, :2 * L], eps, dz, dkl)
    yard = R.posterior(h[:, :2 * L], eps, dz, dkl, dtype=torch.float32)
    hb, hd = _put(h, cuda)
    eb, ed = _put(eps, cuda)
    zb, zd = _put(dz, cuda)
    kd = torch.tensor([float("nan"), dkl, float("nan")], device=cuda)
    ob, z = _band((T, L), torch.float32, cuda)
    klb, kl = _band((1,), torch.float32, cuda)
    gb, dh = _band((T, ld), torch.float32, cuda)                 # dh through the same stride: its padding columns must stay NaN
    ws = _ws("gvf_posterior_workspace_bytes", cuda, T, L)

    def launch(stream):
        sp = _stream_ptr(stream)
        _lib.check(_lib.lib().gvf_posterior_fwd(_p(hd), ld, _p(ed), _p(z), _p(kl), T, L, _p(ws), ws.numel() * 8, sp), "fwd")
        _lib.check(_lib.lib().gvf_posterior_bwd(_p(hd), ld, _p(ed), _p(zd), _p(kd[1:]), _p(dh), ld, T, L, sp), "bwd")
    _twice_and_other_stream(launch, [ob, klb, gb])
    for buf, n in ((hb, T * ld), (eb, T * L), (zb, T * L), (ob, T * L), (klb, 1), (gb, T * ld)):
        assert _bands_nan(buf, n), "a store outside the rows of the call"
    if strided:
        assert bool(torch.isnan(dh[:, 2 * L:]).all()), "the padding columns of dh were written"
    tag, log = f"posterior T{T} L{L} {'strided' if strided else 'contiguous'}", []
    _check(tag, "z", z.cpu(), ref["z"], yard["z"], log)
    _check(tag, "dh", dh.cpu()[:, :2 * L], ref["dh"], yard["dh"], log)
    err, bound = abs(float(kl.cpu()[0]) - float(ref["kl"])), R.kl_bound(h[:, :2 * L], L)
    print(tag, "| kernel/yardstick:", "; ".join(log), f"| kl {float(ref['kl']):.6f} err {err:.2e} bound {bound:.2e} (fp32 torch: "
          f"{abs(float(yard['kl']) - float(ref['kl'])):.2e})")
    assert err <= bound, f"{tag}: |kl - kl64| = {err:.3e} > {bound:.3e}"
    # dz = None: the KL part alone; dkl = None: the sample part alone; they add up to the whole
    only_kl, only_z = torch.empty((T, 2 * L), device=cuda), torch.empty((T, 2 * L), device=cuda)
    _lib.check(_lib.lib().gvf_posterior_bwd(_p(hd), ld, None, None, _p(kd[1:]), _p(only_kl), 2 * L, T, L, None), "bwd kl")
    _lib.check(_lib.lib().gvf_posterior_bwd(_p(hd), ld, _p(ed), _p(zd), None, _p(only_z), 2 * L, T, L, None), "bwd z")
    parts = only_kl.cpu().double() + only_z.cpu().double()
    assert R.rel_l2(parts, ref["dh"]) <= 2 * max(R.rel_l2(yard["dh"], ref["dh"]), 2.0 ** -24)


def test_posterior_autograd(cuda):
    g = torch.Generator().manual_seed(9)
    T, L = 77, 8
    wide = (torch.randn((T, 2 * L + 8), generator=g)).to(cuda).requires_grad_()
    eps = torch.randn((T, L), generator=g).to(cuda)
    w = torch.randn((T, L), generator=g).to(cuda)
    z, kl = S.posterior(wide[:, 4:4 + 2 * L], eps)                  # a column slice: read through its stride
    ((z * w).sum() + 3.0 * kl).backward()
    w64 = wide.detach().double().requires_grad_()
    m, lv = w64[:, 4:4 + L], w64[:, 4 + L:4 + 2 * L]
    ((((m + torch.exp(0.5 * lv) * eps.double()) * w.double()).sum()) + 3.0 * 0.5 * torch.mean(m.pow(2) + lv.exp() - lv - 1)).backward()
    assert R.rel_l2(wide.grad, w64.grad) <= 1e-6 and float(wide.grad[:, :4].abs().max()) == 0
    zz, kk = S.posterior(wide[:, 4:4 + 2 * L], eps)
    gk, = torch.autograd.grad(kk, wide)                               # kl alone: z's gradient arrives as None
    assert torch.isfinite(gk).all() and float(gk.abs().max()) > 0


# ---- regularisers -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kappa", [0.0, 9e-4])
@pytest.mark.parametrize("act", ["exp", "softplus"])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 8264])
def test_gaussian_reg_forward_and_backward(cuda, N, act, kappa):
    g = torch.Generator().manual_seed(N + (7 if act == "exp" else 0))
    softplus = act == "softplus"
    s = torch.randn((N, 3), generator=g) * (6.0 if softplus else 1.0) + (4.0 if softplus else -4.0)
    if softplus:
        s[::5] += 21.0                                           # raw scalings above 20: the linear branch
        assert bool((s > 20).any()) or N < 2
    o = torch.randn((N,), generator=g) * 2
    bs, bo = (0.0113 if softplus else -4.6), -2.1972
    dvol, dopa = 0.7 * N, -1.3 * N
    ref, yard = R.reg(s, o, bs, bo, kappa, softplus, dvol, dopa), R.reg(s, o, bs, bo, kappa, softplus, dvol, dopa, dtype=torch.float32)
    for shift in (0, 1):                                         # shift 1: 4 bytes off a 16-byte boundary, the element-wise path
        sb, sd = _put(s, cuda, shift)
        ob, od = _put(o, cuda, shift)
        gv = torch.tensor([float("nan"), dvol, dopa, float("nan")], device=cuda)
        rb, res = _band((2,), torch.float32, cuda)
        dsb, ds = _band((N, 3), torch.float32, cuda, shift)
        dob, do = _band((N,), torch.float32, cuda, shift)
        ws = _ws("gvf_gaussian_reg_workspace_bytes", cuda, N)
        code = S.ACTIVATIONS[act]

        def launch(stream):
            sp = _stream_ptr(stream)
            _lib.check(_lib.lib().gvf_gaussian_reg_fwd(_p(sd), _p(od), N, bs, bo, kappa, code, _p(res), _p(res[1:]), _p(ws), ws.numel() * 8, sp), "fwd")
            _lib.check(_lib.lib().gvf_gaussian_reg_bwd(_p(sd), _p(od), N, bs, bo, kappa, code, _p(gv[1:]), _p(gv[2:]), _p(ds), _p(do), sp), "bwd")
        _twice_and_other_stream(launch, [rb, dsb, dob])
        for buf, n, sh in ((sb, 3 * N, shift), (ob, N, shift), (rb, 2, 0), (dsb, 3 * N, shift), (dob, N, shift)):
            assert _bands_nan(buf, n, sh), "a store outside the rows of the call"
        tag, log = f"reg N{N} {act} kappa{kappa} shift{shift}", []
        _check(tag, "ds", ds.cpu(), ref["ds"], yard["ds"], log)
        _check(tag, "do", do.cpu().reshape(-1, 1), ref["do"].reshape(-1, 1), yard["do"].reshape(-1, 1), log)
        bv, bop = R.reg_bounds(s, o, bs, bo, kappa, softplus)
        ev, eo = abs(float(res.cpu()[0]) - float(ref["vol"])), abs(float(res.cpu()[1]) - float(ref["opa"]))
        print(tag, "| kernel/yardstick:", "; ".join(log), f"| vol {float(ref['vol']):.4e} err {ev:.2e} bound {bv:.2e} | opa {float(ref['opa']):.4e} "
              f"err {eo:.2e} bound {bop:.2e}")
        assert ev <= bv, f"{tag}: |vol - vol64| = {ev:.3e} > {bv:.3e}"
        assert eo <= bop, f"{tag}: |opa - opa64| = {eo:.3e} > {bop:.3e}"


def test_gaussian_reg_autograd_on_a_gaussian_model(cuda):
    """the operator on a GaussianModel's raw tensors and constants equals the reference's formula on its activated accessors"""
    from gvfdiffusion_amd.representations.gaussian.gaussian_model import GaussianModel
    g = torch.Generator().manual_seed(2)
    for act in ("exp", "softplus"):
        gm = GaussianModel(mininum_kernel_size=9e-4, scaling_bias=0.004, opacity_bias=0.1, scaling_activation=act, device=cuda)
        gm._scaling = (torch.randn((300, 3), generator=g) * 0.5).to(cuda).requires_grad_()
        gm._opacity = torch.randn((300, 1), generator=g).to(cuda).requires_grad_()
        vol, opa = S.gaussian_reg(gm._scaling, gm._opacity, float(gm.scale_bias), float(gm.opacity_bias), gm.mininum_kernel_size, act)
        gs, go = torch.autograd.grad(2.0 * vol + 0.5 * opa, [gm._scaling, gm._opacity])
        vol_t, opa_t = torch.prod(gm.get_scaling, dim=1).mean(), (gm.get_opacity - 1).pow(2).mean()
        ts, to = torch.autograd.grad(2.0 * vol_t + 0.5 * opa_t, [gm._scaling, gm._opacity])
        assert abs(float(vol - vol_t)) <= 1e-5 * float(vol_t) and abs(float(opa - opa_t)) <= 1e-5 * float(opa_t)
        assert R.rel_l2(gs, ts) <= 1e-5 and R.rel_l2(go, to) <= 1e-5 and go.shape == gm._opacity.shape
        v2, _ = S.gaussian_reg(gm._scaling, gm._opacity, float(gm.scale_bias), float(gm.opacity_bias), gm.mininum_kernel_size, act)
        only, = torch.autograd.grad(v2, gm._scaling)                             # one term unused: its gradient arrives as None
        assert R.rel_l2(only * 2.0, torch.autograd.grad(2.0 * torch.prod(gm.get_scaling, dim=1).mean(), gm._scaling)[0]) <= 1e-5


# ---- column sums --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,C", [(1, 1), (63, 100), (64, 256), (65, 768), (4099, 130)])
def test_colsum_and_the_bias_gradient_tap(cuda, rows, C):
    """Accumulated in double: the only fp32 rounding is the result's, |out - sum64| <= 2^-24 |sum64| (plus 2^-50 of the sum of magnitudes for
    the double additions)."""
    g = torch.Generator().manual_seed(rows + C)
    x = torch.randn((rows, C), generator=g) * 3 + 0.25
    xb, xd = _put(x, cuda)
    ob, out = _band((C,), torch.float32, cuda)
    ws = _ws("gvf_colsum_f32_workspace_bytes", cuda, rows, C)

    def launch(stream):
        _lib.check(_lib.lib().gvf_colsum_f32(_p(xd), rows, C, _p(out), _p(ws), ws.numel() * 8, _stream_ptr(stream)), "colsum")
    _twice_and_other_stream(launch, [ob])
    assert _bands_nan(ob, C) and _bands_nan(xb, rows * C)
    ref = x.double().sum(0)
    assert bool(((out.cpu().double() - ref).abs() <= 2.0 ** -24 * ref.abs() + 2.0 ** -50 * x.double().abs().sum(0)).all())
    o = torch.randn((rows, C), generator=g).to(cuda).requires_grad_()
    b = torch.zeros(C, device=cuda, requires_grad=True)
    y = S.bias_grad_tap(o, b)
    assert torch.equal(y, o)
    go, gb = torch.autograd.grad(y, [o, b], xd)
    assert torch.equal(go, xd) and torch.equal(gb, out)
