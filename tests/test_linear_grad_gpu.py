"""Element-wise conformance of a projection's backward (csrc/linear_grad.hip, gvfdiffusion_amd/ops/linear_grad.py) against float64 computed from
the same 16-bit operands (every product of two 16-bit values is exact in float64; the float64 sums run on the device and are exact to
M 2^-53 relative, far below the bound).

Bound of the weight gradient, from the kernel's arithmetic (the form of gemm_ref.accumulation_error): a group of the split accumulates
steps = ceil(ceil(M / 32) / splits) MFMA k-steps, each counted as one fp32 rounding of a partial sum of magnitude at most
S[n][k] = sum_m |dy[m][n] x[m][k]|; the reducer adds `splits` slots, one rounding each; two more are slack for the MFMA's internal order:

    |dW - ref| <= (steps + splits + 2) * 2^-24 * S[n][k]

The bias gradient is the same chain with x replaced by ones (one MFMA against a fragment of ones per k-step, the same reducer), so
|db - ref| <= (steps + splits + 2) * 2^-24 * sum_m |dy[m][n]|.  Every case checks (a) every element of dW and db inside the bound, (b) nothing
outside [N, K] / [N] written (views inside NaN-filled buffers, lddw > K, rows after N), (c) nothing outside [M, N] / [M, K] read (the operands are
views whose padding rows and columns hold NaN), (d) a workspace filled with NaN before the launch, nothing written past its reported size,
(e) the same bits on a second launch.  max |err| / bound is printed per case (python -m pytest -s)."""
import math

import pytest
import torch

import gemm_ref as G
from gvfdiffusion_amd.ops import dit_ops, linear_grad

pytestmark = pytest.mark.gpu
DTYPES = [torch.bfloat16, torch.float16]
SENTINEL16 = 0x7E5A                  # a 16-bit pattern no kernel writes here (fp16: a NaN payload; bf16: 7.2e37)

# (M, N, K, splits): the smallest shapes at which each mechanism can fail
CASES = [(1, 32, 32, 1), (31, 64, 96, 1), (33, 192, 64, 2), (222, 128, 64, 3),
         (40, 128, 128, 4),                                              # more groups than k-steps
         (240, 192, 64, 0), (240, 64, 256, 0), (240, 256, 64, 0),        # the reduced DiT's own shapes
         (1000, 160, 288, 7),                                            # everything partial, the last group short
         (257, 2048, 512, 0), (257, 512, 2048, 0), (4099, 512, 512, 0)]


def _bits(t):
    return t.view(torch.int16) if t.element_size() == 2 else t.view(torch.int32)


def _padded(host, rows_after, cols_after, dev):
    """A device view of `host` (rows, cols) inside a buffer whose extra rows and columns hold NaN."""
    buf = torch.full((host.shape[0] + rows_after, host.shape[1] + cols_after), float("nan"), dtype=host.dtype, device=dev)
    buf[:host.shape[0], :host.shape[1]] = host.to(dev)
    return buf[:host.shape[0], :host.shape[1]]


def wgrad_model(dy, x, splits):
    """(dW reference, dW bound, db reference, db bound) as float64 device tensors; dy [M, N], x [M, K] 16-bit device tensors."""
    M = dy.shape[0]
    d, xx = dy.double(), x.double()
    steps = -(-(-(-M // 32)) // splits)
    c = (steps + splits + 2) * G.U32
    return d.T @ xx, c * (d.abs().T @ xx.abs()), d.sum(0), c * d.abs().sum(0)


_MODEL = {}


def _case(dt, M, N, K, splits, dev):
    """Operands and the float64 model of a case, computed once and shared by its variants (never modified)."""
    key = (dt, M, N, K, splits)
    if key not in _MODEL:
        g = torch.Generator().manual_seed(1000 * M + N + K)
        dy_h = torch.randn((M, N), generator=g).to(dt)
        x_h = torch.randn((M, K), generator=g).to(dt)
        dy, x = _padded(dy_h, 3, 8, dev), _padded(x_h, 2, 16, dev)
        s = splits if splits else linear_grad.wgrad_splits(M, N, K)
        _MODEL[key] = (dy, x, s, wgrad_model(dy.contiguous(), x.contiguous(), s))
    return _MODEL[key]


def _inside(out, ref, bnd, what):
    n_bad, worst = G.excess(out.cpu(), ref.cpu(), bnd.cpu())
    print(f"{what}: max |err| / bound {worst:.3f}")
    assert n_bad == 0, f"{what}: {n_bad} of {ref.numel()} elements outside the bound (worst {worst:.2f} x)"


@pytest.mark.parametrize("with_db", [True, False], ids=["db", "nodb"])
@pytest.mark.parametrize("M,N,K,splits", CASES, ids=lambda v: str(v))
@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
def test_wgrad_elementwise(cuda, dt, M, N, K, splits, with_db):
    dy, x, s, (ref_w, bnd_w, ref_b, bnd_b) = _case(dt, M, N, K, splits, cuda)
    assert dy.stride(0) == N + 8 and x.stride(0) == K + 16
    nan = float("nan")
    wbuf = torch.full((N + 2, K + 8), nan, dtype=torch.float32, device=cuda)
    bbuf = torch.full((N + 8,), nan, dtype=torch.float32, device=cuda)
    need = linear_grad.wgrad_workspace_bytes(M, N, K, splits)
    assert need == ((s * (N * K + N) * 4 + 255) // 256) * 256
    ws = torch.full((need + 256,), 0xFF, dtype=torch.uint8, device=cuda)       # (four 0xFF bytes: an fp32 NaN)

    def launch():
        ws.fill_(0xFF)
        linear_grad.wgrad(dy, x, bias=with_db, splits=splits, out=wbuf[:N, :K], out_bias=bbuf[:N] if with_db else None, workspace=ws[:need])
        torch.cuda.synchronize()

    launch()
    what = f"wgrad {dt} M{M} N{N} K{K} splits {splits or 'auto'}={s}{' +db' if with_db else ''}"
    dw = wbuf[:N, :K].clone()
    db = bbuf.clone()
    _inside(dw, ref_w, bnd_w, what + " dW")
    if with_db:
        _inside(db[:N], ref_b, bnd_b, what + " db")
    # (b) the guard bands: still NaN, bit for bit
    mask = torch.ones(wbuf.shape, dtype=torch.bool, device=cuda)
    mask[:N, :K] = False
    assert bool((_bits(wbuf)[mask] == _bits(torch.full_like(wbuf, nan))[mask]).all()), f"{what}: a store outside [N, K] of dW"
    assert bool(torch.isnan(db[N:] if with_db else db).all()), f"{what}: a store outside db"
    assert bool((ws[need:] == 0xFF).all()), f"{what}: a store past the workspace"
    # (e) the same bits again (the workspace poisoned again first)
    wbuf[:N, :K].fill_(nan)
    launch()
    assert torch.equal(_bits(wbuf[:N, :K].contiguous()), _bits(dw)), f"{what}: a second launch gave other bits"
    if with_db:
        assert torch.equal(_bits(bbuf[:N]), _bits(db[:N]))


def test_wgrad_empty_operand_gives_zeros(cuda):
    dw, db = linear_grad.wgrad(torch.zeros((0, 64), dtype=torch.bfloat16, device=cuda), torch.zeros((0, 32), dtype=torch.bfloat16, device=cuda))
    assert dw.shape == (64, 32) and db.shape == (64,) and not bool(dw.any()) and not bool(db.any())


def _special_values(dt):
    """fp32 values whose rounding to `dt` is a tie, denormal, out of range or not a number."""
    p = 8 if dt == torch.bfloat16 else 11                    # mantissa bits incl. the hidden one
    h = 2.0 ** -p                                            # half a step at 1.0
    v = [1 + h, 1 + 3 * h, -(1 + h), -(1 + 3 * h), 1 + h * (1 + 2.0 ** -10), 1 + h * (1 - 2.0 ** -10),      # ties (to even) and their neighbours
         1e-40, -1e-40, 1.4e-45, 2.0 ** -126, 2.0 ** -133, 3 * 2.0 ** -134,                                     # fp32 denormals / bf16 denormals and a tie
         2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25, 2.0 ** -25 * (1 + 2.0 ** -10), 6e-8, 1e-6, 6.1e-5,             # fp16 denormals, ties at the bottom
         65504.0, 65519.0, 65520.0, 1e6, -1e6, 3.38e38, 3.4e38,                                                 # largest finite / overflow to inf
         float("inf"), float("-inf"), float("nan"), 0.0, -0.0]
    return torch.tensor(v, dtype=torch.float32)


@pytest.mark.parametrize("N,K", [(64, 64), (192, 64), (200, 72), (2048, 512)], ids=lambda v: str(v))
@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
def test_cast_transpose_bit_exact(cuda, dt, N, K):
    """Both images against Tensor.to: the same bits wherever the value is a number; where it is NaN, a NaN (its payload is nobody's contract).
    The master is a view with an odd row stride whose padding holds NaN; the images are views inside sentinel-filled buffers with leading dimensions
    8 beyond the rounded extent: their padding columns must be zero, the row after the last untouched."""
    g = torch.Generator().manual_seed(N + K)
    w_h = torch.randn((N, K), generator=g)
    sp = _special_values(dt)
    idx = torch.randperm(N * K, generator=g)[:4 * sp.numel()]
    w_h.view(-1)[idx] = sp.repeat(4)
    w = _padded(w_h, 1, 3, cuda)
    ld_k, ld_n = (K + 7) // 8 * 8 + 8, (N + 7) // 8 * 8 + 8
    buf = torch.full((N + 1, ld_k), SENTINEL16, dtype=torch.int16, device=cuda).view(dt)
    buft = torch.full((K + 1, ld_n), SENTINEL16, dtype=torch.int16, device=cuda).view(dt)
    w16, w16t = linear_grad.cast_transpose(w, dt, out=(buf[:N], buft[:K]))
    torch.cuda.synchronize()
    ref = w.contiguous().to(dt)
    for got, want, name in ((w16, ref, "image"), (w16t, ref.t().contiguous(), "transposed image")):
        assert got.shape == want.shape
        num = ~torch.isnan(want)
        assert int((~num).sum()) == 4
        assert bool(torch.isnan(got[~num]).all()), f"{name}: a NaN was cast to a number"
        diff = (_bits(got.contiguous()) != _bits(want)) & num
        assert not bool(diff.any()), f"{name} {dt} {N}x{K}: {int(diff.sum())} elements differ from Tensor.to, first {got[diff][:4].tolist()} vs {want[diff][:4].tolist()}"
    assert not bool(_bits(buf)[:N, K:].any()) and not bool(_bits(buft)[:K, N:].any()), "padding columns must be zero"
    assert bool((_bits(buf)[N] == SENTINEL16).all()) and bool((_bits(buft)[K] == SENTINEL16).all()), "a store past the last row"
    # the default call: rows padded to 8 elements, views of the extent
    a, b = linear_grad.cast_transpose(w, dt)
    assert a.shape == (N, K) and b.shape == (K, N) and torch.equal(_bits(a.contiguous()), _bits(w16.contiguous()))
    assert torch.equal(_bits(b.contiguous()), _bits(w16t.contiguous()))


@pytest.mark.parametrize("shape,N", [((240, 64), 192), ((222, 64), 128), ((6, 40, 64), 128)], ids=["240x192x64", "222x128x64", "6x40x64-3d"])
@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
def test_linear_through_autograd(cuda, dt, shape, N, monkeypatch):
    K = shape[-1]
    M = math.prod(shape[:-1])
    g = torch.Generator().manual_seed(M + N)
    w = (torch.randn((N, K), generator=g) / math.sqrt(K)).to(cuda).requires_grad_(True)
    b = torch.randn((N,), generator=g).to(cuda).requires_grad_(True)
    x = torch.randn(shape, generator=g).to(dt).to(cuda).requires_grad_(True)
    dy = torch.randn(shape[:-1] + (N,), generator=g).to(dt).to(cuda)
    y = linear_grad.linear(x, w, b, dtype=dt)
    assert y.shape == dy.shape and y.dtype == dt
    w16 = w.detach().to(dt)
    y_ref = dit_ops.gemm(x.detach().reshape(M, K), w16, b.detach(), torch.empty((M, N), dtype=dt, device=cuda), dit_ops.EPI_STORE_16)
    assert torch.equal(_bits(y.detach().reshape(M, N).contiguous()), _bits(y_ref)), "the forward is gvf_gemm on the cast weight"
    y.backward(dy)
    torch.cuda.synchronize()
    assert x.grad.dtype == dt and x.grad.shape == x.shape and w.grad.dtype == torch.float32 and b.grad.dtype == torch.float32
    what = f"linear {dt} {tuple(shape)} -> {N}"
    ref_x, bnd_x = G.model(dy.reshape(M, N).cpu(), w16.t().contiguous().cpu(), None, G.EPI_STORE_16)          # A = dY, W = W16T [K][N]
    n_bad, worst = G.excess(x.grad.reshape(M, K).cpu(), ref_x, bnd_x)
    print(f"{what} dX: max |err| / bound {worst:.3f}")
    assert n_bad == 0
    s = linear_grad.wgrad_splits(M, N, K)
    ref_w, bnd_w, ref_b, bnd_b = wgrad_model(dy.reshape(M, N), x.detach().reshape(M, K), s)
    _inside(w.grad, ref_w, bnd_w, what + " dW")
    _inside(b.grad, ref_b, bnd_b, what + " db")

    # what needs no gradient is not computed
    calls = {"gemm": 0, "wgrad": 0}
    real_gemm, real_wgrad = dit_ops.gemm, linear_grad.wgrad
    monkeypatch.setattr(dit_ops, "gemm", lambda *a, **k: (calls.__setitem__("gemm", calls["gemm"] + 1), real_gemm(*a, **k))[1])
    monkeypatch.setattr(linear_grad, "wgrad", lambda *a, **k: (calls.__setitem__("wgrad", calls["wgrad"] + 1), real_wgrad(*a, **k))[1])
    x2 = x.detach().clone()                                   # requires_grad False
    w.grad = b.grad = None
    linear_grad.linear(x2, w, b, dtype=dt).backward(dy)
    assert x2.grad is None and calls == {"gemm": 1, "wgrad": 1}, calls
    assert w.grad is not None and b.grad is not None
    _inside(w.grad, ref_w, bnd_w, what + " dW (x frozen)")
    calls.update(gemm=0, wgrad=0)
    x3 = x.detach().clone().requires_grad_(True)
    wf, bf = w.detach().clone(), b.detach().clone()           # frozen parameters
    linear_grad.linear(x3, wf, bf, dtype=dt).backward(dy)
    assert wf.grad is None and bf.grad is None and calls == {"gemm": 2, "wgrad": 0}, calls
    assert torch.equal(_bits(x3.grad), _bits(x.grad))
    # a non-contiguous input and gradient: made contiguous, the same bits
    if len(shape) == 2:
        xt = x.detach().t().contiguous().t().requires_grad_(True)
        assert not xt.is_contiguous()
        w.grad = b.grad = None
        yt = linear_grad.linear(xt, w, b, dtype=dt)
        yt.backward(dy.t().contiguous().t())
        assert torch.equal(_bits(xt.grad.contiguous()), _bits(x.grad))


def test_linear_refuses_what_the_gemm_cannot_contract(cuda):
    x = torch.zeros((8, 48), dtype=torch.bfloat16, device=cuda)
    with pytest.raises(ValueError):
        linear_grad.linear(x, torch.zeros((64, 48), device=cuda))                  # K % 32 != 0
    with pytest.raises(ValueError):
        linear_grad.linear(torch.zeros((8, 64), dtype=torch.bfloat16, device=cuda), torch.zeros((72, 64), device=cuda))      # N % 32 != 0
    with pytest.raises(ValueError):
        linear_grad.linear(torch.zeros((8, 64), dtype=torch.float16, device=cuda), torch.zeros((64, 64), device=cuda), dtype=torch.bfloat16)


def test_weight_images_are_cast_once_per_cache(cuda, monkeypatch):
    n = {"cast": 0}
    real = linear_grad.cast_transpose
    monkeypatch.setattr(linear_grad, "cast_transpose", lambda *a, **k: (n.__setitem__("cast", n["cast"] + 1), real(*a, **k))[1])
    w = torch.randn((64, 32), device=cuda, requires_grad=True)
    x = torch.randn((16, 32), device=cuda).to(torch.bfloat16)
    cache = {}
    y1 = linear_grad.linear(x, w, dtype=torch.bfloat16, cache=cache)
    y2 = linear_grad.linear(x, w, dtype=torch.bfloat16, cache=cache)
    assert n["cast"] == 1 and torch.equal(y1, y2)
    linear_grad.linear(x, w, dtype=torch.bfloat16)
    assert n["cast"] == 2
