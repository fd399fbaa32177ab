"""The DiT training kernels (csrc/dit_train.hip) against the float64 formulas of tests/dit_train_ref.py on the same rounded inputs, both
operand types: every output by relative L2 over the whole tensor and over its worst block of 32 rows, the bar being TWICE the error of the
fp32 yardstick (the same formulas as a naive fp32 composition with the kernels' rounding points) -- room for another summation order, not
for another algorithm (the convention of tests/test_attn_bwd_gpu.py).  A gradient that is zero in exact arithmetic is held element-wise
to a stated fp32 floor.  Also: guard rows around every output, NaN in every padding the contract allows, the same bits on a second launch
and on another stream.  The entry points are called through ctypes on buffers of the test's own (the operators allocate theirs)."""
import ctypes

import pytest
import torch

import dit_train_ref as R
from gvfdiffusion_amd import _lib
from gvfdiffusion_amd.ops import dit_ops, dit_train as T

pytestmark = pytest.mark.gpu
DTYPES = [torch.bfloat16, torch.float16]
GUARD = 3
SENT = 12345.0
SHAPES = [(256, 37, 10), (512, 1, 1), (512, 130, 48), (1024, 9, 4), (64, 37, 10), (100, 6, 4), (1028, 41, 7)]


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _guarded(rows, cols, dtype, dev):
    """(buffer with GUARD sentinel rows on both sides, the view of the rows in between)"""
    buf = torch.full((rows + 2 * GUARD, cols), SENT, dtype=dtype, device=dev)
    return buf, buf[GUARD:GUARD + rows]


def _guards_intact(buf, rows):
    g = torch.cat([buf[:GUARD], buf[GUARD + rows:]]).float()
    return bool((g == torch.tensor(SENT, dtype=buf.dtype).float().item()).all())


def _ws(name, dev, *dims):
    nb = ctypes.c_size_t(0)
    assert getattr(_lib.lib(), name)(*dims, ctypes.byref(nb)) == _lib.GVF_OK
    return torch.full((int(nb.value) // 4 + 4,), float("nan"), device=dev)          # NaN: a slot read before it is written shows


def _stream_ptr(s):
    return ctypes.c_void_p(s.cuda_stream)


def _twice_and_other_stream(launch, bufs):
    """launch(stream) three times: current stream, again, and a side stream; every buffer must hold the same bits each time."""
    cur = torch.cuda.current_stream()
    launch(cur)
    torch.cuda.synchronize()
    first = [b.clone() for b in bufs]
    launch(cur)
    torch.cuda.synchronize()
    for b, f in zip(bufs, first):
        assert torch.equal(b.view(torch.uint8), f.view(torch.uint8)), "a second launch gave other bits"
    side = torch.cuda.Stream()
    side.wait_stream(cur)
    with torch.cuda.stream(side):
        launch(side)
    side.synchronize()
    for b, f in zip(bufs, first):
        assert torch.equal(b.view(torch.uint8), f.view(torch.uint8)), "another stream gave other bits"


def _check(tag, name, got, ref64, yard, bar_log):
    """kernel error <= 2 x yardstick error, whole tensor and worst 32-row block"""
    got, ref64, yard = (t.reshape(t.shape[0], -1) for t in (got, ref64, yard))
    assert torch.isfinite(got.float()).all() or not torch.isfinite(ref64).all(), f"{tag} {name}: non-finite output"
    e, ey = R.rel_l2(got, ref64), R.rel_l2(yard, ref64)
    w, wy = R.worst_rows(got, ref64), R.worst_rows(yard, ref64)
    bar_log.append(f"{name} {e:.2e}/{ey:.2e} blk {w:.2e}/{wy:.2e}")
    assert e <= 2 * ey, f"{tag} {name}: rel L2 {e:.3e} > 2 x yardstick {ey:.3e}"
    assert w <= 2 * wy, f"{tag} {name}: worst 32-row block {w:.3e} > 2 x yardstick {wy:.3e}"


def _ln_rows(C, rows, g):
    """the adversarial rows of tests/test_elem_conformance_gpu.py"""
    x = torch.randn((rows, C), generator=g) * 2 + 0.5
    x[0:3] += 200.0                                               # |mean| = 100 x std
    for r, v in zip(range(3, min(6, rows)), (3.0, -0.37, 0.0)):
        x[r] = v                                                  # constant rows: eps decides
    x[6:8, 1::29] = 1e4                                           # huge elements
    return x


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("with_dres", [True, False], ids=["dres", "nodres"])
@pytest.mark.parametrize("mode", ["affine", "adaln", "both", "neither"])
@pytest.mark.parametrize("C,rows,rpg", SHAPES)
def test_layernorm_modulate_backward(cuda, dt, mode, with_dres, C, rows, rpg):
    g = torch.Generator().manual_seed(C * 7 + rows)
    x = _ln_rows(C, rows, g)
    G = (rows + rpg - 1) // rpg
    ld = 2 * C + 12                                               # [4 | shift C | 4 | scale C | 4], NaN in the padding
    mod = torch.full((G, ld), float("nan"))
    mod[:, 4:4 + C] = torch.randn((G, C), generator=g) * 0.3
    mod[:, 8 + C:8 + 2 * C] = torch.randn((G, C), generator=g) * 0.3
    mod[-1, 8 + C:8 + C + C // 2] = -1.0                          # 1 + scale = 0 in half of the last group's columns
    lw, lb = 1 + 0.1 * torch.randn((C,), generator=g), 0.1 * torch.randn((C,), generator=g)
    dy = torch.randn((rows, C), generator=g).to(dt)
    dy[:, 5:9] = 0                                                # columns whose four sums are zero in exact arithmetic
    dres = torch.randn((rows, C), generator=g)
    has_mod, has_aff = mode in ("adaln", "both"), mode in ("affine", "both")
    shift, scale = (mod[:, 4:4 + C], mod[:, 8 + C:8 + 2 * C]) if has_mod else (None, None)
    w, b = (lw, lb) if has_aff else (None, None)
    kw = dict(dres=dres if with_dres else None, w=w, b=b, shift=shift, scale=scale, rpg=rpg)
    ref = R.ln_mod(x, dy.float(), **kw)
    yard = R.ln_mod(x, dy.float(), dtype=torch.float32, lp=dt, **kw)

    dev = cuda
    xd, dyd, md = x.to(dev), dy.to(dev), mod.to(dev)
    dresd = dres.to(dev) if with_dres else None
    wd, bd = (lw.to(dev), lb.to(dev)) if has_aff else (None, None)
    scd, shd = (md[:, 8 + C:], md[:, 4:]) if has_mod else (None, None)
    ybuf, y = _guarded(rows, C, dt, dev)
    dxbuf, dx = _guarded(rows, C, torch.float32, dev)
    sbuf, dsh = _guarded(G, C, torch.float32, dev)
    cbuf, dsc = _guarded(G, C, torch.float32, dev)
    wbuf, dw = _guarded(1, C, torch.float32, dev)
    bbuf, db = _guarded(1, C, torch.float32, dev)
    ws = _ws("gvf_ln_mod_bwd_workspace_bytes", dev, rows, C, rpg if has_mod else 0)
    code = dit_ops.dt_code(dt)

    def launch(stream):
        sp = _stream_ptr(stream)
        _lib.check(_lib.lib().gvf_layernorm_modulate(code, _p(xd), _p(y), rows, C, 1e-6, _p(wd), _p(bd), _p(shd), _p(scd), ld, rpg, sp), "fwd")
        _lib.check(_lib.lib().gvf_ln_mod_bwd(code, _p(xd), _p(dyd), _p(dresd), _p(dx), rows, C, 1e-6, _p(wd), _p(bd), _p(scd), ld, rpg,
                                             _p(dsh) if has_mod else None, _p(dsc) if has_mod else None, _p(dw) if has_aff else None,
                                             _p(db) if has_aff else None, _p(ws), ws.numel() * 4, sp), "bwd")
    _twice_and_other_stream(launch, [ybuf, dxbuf, sbuf, cbuf, wbuf, bbuf])
    for buf, n in ((ybuf, rows), (dxbuf, rows), (sbuf, G), (cbuf, G), (wbuf, 1), (bbuf, 1)):
        assert _guards_intact(buf, n), "a store outside the rows of the call"
    if not has_mod:
        assert bool((sbuf == SENT).all()) and bool((cbuf == SENT).all()), "dshift / dscale written without a scale"
    if not has_aff:
        assert bool((wbuf == SENT).all()) and bool((bbuf == SENT).all()), "dw / db written without an affine pair"
    tag, log = f"ln_bwd C{C} rows{rows} rpg{rpg} {mode} {'dres' if with_dres else 'nodres'} {dt}", []
    _check(tag, "y", y.cpu(), ref["y"], yard["y"], log)
    _check(tag, "dx", dx.cpu(), ref["dx"], yard["dx"], log)
    outs = ([("dshift", dsh), ("dscale", dsc)] if has_mod else []) + ([("dw", dw), ("db", db)] if has_aff else [])
    for name, t in outs:
        got = t.cpu().reshape(-1, C)
        _check(tag, name, got, ref[name].reshape(-1, C), yard[name].reshape(-1, C), log)
        # the columns where dy is zero: sums of exact zeros, floor 0
        assert bool((got.reshape(-1, C)[:, 5:9] == 0).all()), f"{tag} {name}: a sum of zeros is not zero"
    print(tag, "| kernel/yardstick:", "; ".join(log))


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("C", [512, 100])
def test_layernorm_backward_of_a_constant_gradient_is_zero_to_the_fp32_floor(cuda, dt, C):
    """Without affine and modulation, dy constant along a row gives g - mean(g) = 0 and mean(g xh) = c mean(xh) = 0: dx is zero in exact
    arithmetic.  Held element-wise: |dx| <= 2^-18 rstd |c| (the sums of C <= 1024 equal terms and of xh are each good to a few ulps of
    2^-24; 64 of them is generous and still 4 decimal orders below a wrong formula)."""
    rows = 21
    g = torch.Generator().manual_seed(C)
    x = (torch.randn((rows, C), generator=g) * 2 + 0.5).to(cuda)
    c = torch.randn((rows, 1), generator=g).to(dt)
    dy = c.expand(rows, C).contiguous().to(cuda)
    dx = torch.full((rows, C), SENT, device=cuda)
    _lib.check(_lib.lib().gvf_ln_mod_bwd(dit_ops.dt_code(dt), _p(x), _p(dy), None, _p(dx), rows, C, 1e-6, None, None, None, 0, 0, None, None, None, None,
                                         None, 0, None), "bwd")
    rstd = R.ln_mod(x.cpu(), dy.cpu().float())["rstd"]
    floor = 2.0 ** -18 * rstd * c.double().abs()
    assert bool((dx.cpu().double().abs() <= floor).all()), float((dx.cpu().double().abs() / floor).max())


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("gated", [True, False], ids=["gate", "nogate"])
@pytest.mark.parametrize("C,rows,rpg", SHAPES)
def test_gate_residual_forward_and_backward(cuda, dt, gated, C, rows, rpg):
    g = torch.Generator().manual_seed(C * 3 + rows)
    G = (rows + rpg - 1) // rpg
    ld = C + 8                                                    # [4 | gate C | 4], NaN in the padding
    tab = torch.full((G, ld), float("nan"))
    tab[:, 4:4 + C] = torch.randn((G, C), generator=g)
    x, dout = torch.randn((rows, C), generator=g), torch.randn((rows, C), generator=g)
    h = (torch.randn((rows, C), generator=g) * 3).to(dt)
    dout[:, 2:4] = 0                                              # dgate columns that are zero in exact arithmetic
    gate = tab[:, 4:4 + C] if gated else None
    ref = R.gate(x, h.float(), dout, gate, rpg)
    yard = R.gate(x, h.float(), dout, gate, rpg, dtype=torch.float32, lp=dt)
    dev = cuda
    xd, hd, dd, td = x.to(dev), h.to(dev), dout.to(dev), tab.to(dev)
    gd = td[:, 4:] if gated else None
    obuf, out = _guarded(rows, C, torch.float32, dev)
    hbuf, dh = _guarded(rows, C, dt, dev)
    gbuf, dgate = _guarded(G, C, torch.float32, dev)
    ws = _ws("gvf_gate_residual_bwd_workspace_bytes", dev, rows, C, rpg if gated else 0)
    code = dit_ops.dt_code(dt)

    def launch(stream):
        sp = _stream_ptr(stream)
        _lib.check(_lib.lib().gvf_gate_residual_fwd(code, _p(xd), _p(hd), _p(gd), ld, rpg, _p(out), rows, C, sp), "fwd")
        _lib.check(_lib.lib().gvf_gate_residual_bwd(code, _p(dd), _p(hd) if gated else None, _p(gd), ld, rpg, _p(dh), _p(dgate) if gated else None, rows, C,
                                                    _p(ws) if gated else None, ws.numel() * 4 if gated else 0, sp), "bwd")
    _twice_and_other_stream(launch, [obuf, hbuf, gbuf])
    for buf, n in ((obuf, rows), (hbuf, rows), (gbuf, G)):
        assert _guards_intact(buf, n), "a store outside the rows of the call"
    tag, log = f"gate C{C} rows{rows} rpg{rpg} {'gate' if gated else 'nogate'} {dt}", []
    # out = x + gate * h: one product and one sum of exact fp32 operands -- the float64 result rounded twice at the most
    _check(tag, "dh", dh.cpu(), ref["dh"], yard["dh"], log)
    e = (out.cpu().double() - ref["out"]).abs()
    assert bool((e <= 2.0 ** -23 * (x.double().abs() + (ref["out"] - x.double()).abs())).all()), f"{tag}: out off by more than two roundings"
    if gated:
        _check(tag, "dgate", dgate.cpu(), ref["dgate"], yard["dgate"], log)
        assert bool((dgate.cpu()[:, 2:4] == 0).all()), f"{tag}: a sum of zeros is not zero"
    else:
        assert bool((gbuf == SENT).all()), "dgate written without a gate"
    print(tag, "| kernel/yardstick:", "; ".join(log))


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("packed", [False, True], ids=["contiguous", "packed_qkv"])
@pytest.mark.parametrize("rows,H,d", [(1, 1, 32), (37, 2, 32), (130, 16, 32), (37, 3, 64)])
def test_rmsnorm_heads_forward_and_backward(cuda, dt, packed, rows, H, d):
    g = torch.Generator().manual_seed(rows * 5 + H + d)
    HD = H * d
    gamma = 1 + 0.2 * torch.randn((H, d), generator=g)
    dy = torch.randn((rows, H, d), generator=g).to(dt)
    zero_row, big_row = (rows // 2, rows - 1) if rows > 1 else (None, 0)

    def rows_of(seed_scale):
        x = torch.randn((rows, H, d), generator=g) * seed_scale
        x[big_row] = torch.randn((H, d), generator=g) * 1e4          # a row of magnitude 1e4
        if zero_row is not None:
            x[zero_row] = 0                                          # an all-zero row: dx = u / 1e-12, what torch gives
        return x.to(dt)
    slices = [rows_of(1.0), rows_of(0.5)] if packed else [rows_of(1.0)]
    dev = cuda
    if packed:
        qkv = torch.full((rows, 3 * HD), float("nan"), dtype=dt, device=dev)     # [q | k | v]: v stays NaN, never read
        qkv[:, :HD], qkv[:, HD:2 * HD] = slices[0].reshape(rows, HD).to(dev), slices[1].reshape(rows, HD).to(dev)
        views, ldx = [qkv[:, :HD], qkv[:, HD:2 * HD]], 3 * HD
    else:
        views, ldx = [slices[0].reshape(rows, HD).to(dev)], HD
    gd, dyd = gamma.to(dev), dy.to(dev)
    code = dit_ops.dt_code(dt)
    for xi, (x16, xv) in enumerate(zip(slices, views)):
        ref = R.rms(x16.float(), dy.float(), gamma)
        yard = R.rms(x16.float(), dy.float(), gamma, dtype=torch.float32, lp=dt)
        ybuf, y = _guarded(rows, HD, dt, dev)
        xbuf, dx = _guarded(rows, HD, dt, dev)
        gbuf, dgamma = _guarded(1, HD, torch.float32, dev)
        ws = _ws("gvf_rmsnorm_heads_bwd_workspace_bytes", dev, rows, H, d)

        def launch(stream):
            sp = _stream_ptr(stream)
            _lib.check(_lib.lib().gvf_rmsnorm_heads_fwd(code, _p(xv), ldx, _p(gd), _p(y), HD, rows, H, d, sp), "fwd")
            _lib.check(_lib.lib().gvf_rmsnorm_heads_bwd(code, _p(xv), ldx, _p(dyd), HD, _p(gd), _p(dx), HD, _p(dgamma), rows, H, d, _p(ws), ws.numel() * 4, sp), "bwd")
        _twice_and_other_stream(launch, [ybuf, xbuf, gbuf])
        for buf, n in ((ybuf, rows), (xbuf, rows), (gbuf, 1)):
            assert _guards_intact(buf, n), "a store outside the rows of the call"
        tag, log = f"rms rows{rows} H{H} d{d} {'packed' if packed else 'contiguous'}[{xi}] {dt}", []
        got_dx = dx.cpu().reshape(rows, H, d)
        if zero_row is not None:
            # u / 1e-12 leaves the 16-bit range in fp16 (inf) and stays finite in bf16: in both cases exactly the rounded float64 value
            want = ref["dx"][zero_row].to(dt)
            assert torch.equal(got_dx[zero_row].view(torch.int16), want.view(torch.int16)) or R.rel_l2(got_dx[zero_row], want) <= 2 ** -7, f"{tag}: the all-zero row"
            assert float(got_dx[zero_row].float().abs().max()) > 1e9
        keep = [r for r in range(rows) if r != zero_row]
        _check(tag, "y", y.cpu().reshape(rows, H, d), ref["y"], yard["y"], log)
        _check(tag, "dx", got_dx[keep], ref["dx"][keep], yard["dx"][keep], log)
        _check(tag, "dgamma", dgamma.cpu().reshape(1, HD), ref["dgamma"].reshape(1, HD), yard["dgamma"].reshape(1, HD), log)
        print(tag, "| kernel/yardstick:", "; ".join(log))
    if packed:
        assert bool(torch.isnan(qkv[:, 2 * HD:].float()).all()), "the v slice of the packed buffer was written"


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
def test_operators_through_autograd_on_chunk_views(cuda, dt):
    """The three autograd operators on what the training forward hands them -- chunk views of a [B, 6C] modulation tensor, the unbind slices
    of a packed qkv projection -- against float64 autograd of the torch composition, with the gradients flowing back into the packed
    tensors; the forward under grad equals the no-grad inference kernel bit for bit; dx of gate_residual is the incoming tensor itself."""
    B, TN, C, H, d = 2, 37, 512, 16, 32
    rows = B * TN
    g = torch.Generator().manual_seed(11)
    x = torch.randn((B, TN, C), generator=g).to(cuda).requires_grad_()
    mod = (0.3 * torch.randn((B, 6 * C), generator=g)).to(cuda).requires_grad_()
    sh, sc, gt = mod.chunk(6, dim=1)[:3]
    y, xres = T.layernorm_modulate(x, shift=sh, scale=sc, rows_per_group=TN, dtype=dt, return_residual=True)
    with torch.no_grad():
        y0 = torch.empty((rows, C), dtype=dt, device=cuda)
        dit_ops.layernorm_modulate(x.detach().reshape(rows, C), y0, 1e-6, None, None, sh.detach(), sc.detach(), 6 * C, TN)
    assert torch.equal(y.detach().reshape(rows, C).view(torch.int16), y0.view(torch.int16))
    qkv = torch.randn((B, TN, 3 * C), generator=g).to(cuda).to(dt).requires_grad_()
    q, k, v = qkv.reshape(B, TN, 3, H, d).unbind(dim=2)
    gq = (1 + 0.1 * torch.randn((H, d), generator=g)).to(cuda).requires_grad_()
    qn = T.rmsnorm_heads(q, gq)
    h = (y.float() * 0.5 + qn.reshape(B, TN, C).float()).to(dt)
    out = T.gate_residual(xres, h, gt, TN)
    wgt = torch.randn((B, TN, C), generator=g).to(cuda)
    (out * wgt).sum().backward()
    # float64 reference of the same graph
    x64, mod64, qkv64, gq64 = (t.detach().double().requires_grad_() for t in (x, mod, qkv, gq))
    sh6, sc6, gt6 = mod64.chunk(6, dim=1)[:3]
    y6 = torch.nn.functional.layer_norm(x64, (C,), None, None, 1e-6) * (1 + sc6[:, None]) + sh6[:, None]
    q6 = qkv64.reshape(B, TN, 3, H, d).unbind(dim=2)[0]
    qn6 = torch.nn.functional.normalize(q6, dim=-1) * gq64 * d ** 0.5
    out6 = x64 + gt6[:, None] * (y6 * 0.5 + qn6.reshape(B, TN, C))
    (out6 * wgt.double()).sum().backward()
    eps16 = 2.0 ** -8 if dt == torch.bfloat16 else 2.0 ** -11
    # three 16-bit roundings sit between the float64 graph and this one (y, qn, h): a few units of the type's epsilon in relative L2
    for name, a, b in (("x", x.grad, x64.grad), ("mod", mod.grad, mod64.grad), ("qkv", qkv.grad, qkv64.grad), ("gamma", gq.grad, gq64.grad)):
        e = R.rel_l2(a, b)
        print(f"autograd {dt} d{name}: rel L2 {e:.2e} (type epsilon {eps16:.1e})")
        assert e <= 4 * eps16, (name, e)
    assert float(mod.grad[:, 3 * C:].abs().max()) == 0 and float(qkv.grad[..., C:].abs().max()) == 0
    # the residual gradient is handed through: dx of gate_residual is the incoming tensor
    dout = torch.randn((rows, C), generator=g).to(cuda)
    hh = h.detach().requires_grad_()
    xx = x.detach().requires_grad_()
    o2 = T.gate_residual(xx, hh)
    dxx, = torch.autograd.grad(o2, xx, dout.reshape(B, TN, C))
    assert dxx.data_ptr() == dout.data_ptr()
