"""LPIPS (VGG16) on the MI355X: every layer kernel alone against fp64 of the same 16-bit operands (tests/lpips_ref.py, bounds from
tests/gemm_ref.py), then the whole operator against the fp64 composition with the reference's own bf16-autocast deviation as yardstick."""
import numpy as np
import pytest
import torch

import lpips_ref as R
from gemm_ref import _round_bound, excess
from gvfdiffusion_amd import synthetic
from gvfdiffusion_amd.ops import image_loss as IL
from gvfdiffusion_amd.ops import lpips as LP
from gvfdiffusion_amd.renderers import GaussianRenderer

pytestmark = pytest.mark.gpu
DTYPES = [torch.float16, torch.bfloat16]
IDS = ["fp16", "bf16"]
CONV_SHAPES = [(2, 9, 21, 64, 64), (1, 17, 33, 64, 128), (1, 5, 7, 512, 512), (1, 2, 3, 512, 512), (1, 1, 1, 512, 512)]     # N, H, W, Cin, Cout
E2E_SHAPES = [(2, 3, 40, 56), (2, 3, 37, 50), (2, 3, 16, 16)]
SEED = 11


def u(stream, shape, lo=-1.0, hi=1.0):
    return torch.from_numpy(R.hash_uniform(SEED, stream, int(np.prod(shape))).reshape(shape) * (hi - lo) + lo).float()


def conv_weight(stream, cout, cin):
    return u(stream, (cout, cin, 3, 3)) * (6.0 / (9 * cin)) ** 0.5


def activation(stream, shape, dt):
    """A stored ReLU output: about half of it exactly zero."""
    return torch.relu(u(stream, shape)).to(dt)


def check(out, ref, bnd, what):
    bad, ratio = excess(out.cpu(), ref, bnd)
    print(f"{what}: {out.numel()} elements, {bad} outside, worst |err| / bound {ratio:.3f}")
    assert torch.isfinite(out).all() and bad == 0, what


# ---- convolution -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", CONV_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_conv3x3_forward(cuda, shape, dt):
    N, H, W, cin, cout = shape
    a = u(1, (N, H, W, cin)).to(dt)
    w, b = conv_weight(2, cout, cin), u(3, (cout,), -0.05, 0.05)
    img = LP.pack_conv(w.to(cuda), LP.PACK_FWD, dt)
    out = LP.conv3x3(a.to(cuda), img, cout, bias=b.to(cuda), relu=True)
    ref, bnd = R.conv_model(a, w.to(dt), bias=b, relu=True)
    assert float((ref > 0).double().mean()) > 0.2
    check(out, ref, bnd, f"conv3x3 forward {shape} {dt}")


@pytest.mark.parametrize("mask_dt", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", CONV_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_conv3x3_input_gradient(cuda, shape, mask_dt):
    """The same kernel on the DGRAD image: bf16 operands, an addend and a mask taken from a stored activation of the forward type."""
    N, H, W, cin, cout = shape
    bf = torch.bfloat16
    z = (u(4, (N, H, W, cout)) * 1e-4).to(bf)
    w = conv_weight(2, cout, cin)
    addend = (u(5, (N, H, W, cin)) * 1e-4).to(bf)
    mask = activation(6, (N, H, W, cin), mask_dt)
    img = LP.pack_conv(w.to(cuda), LP.PACK_DGRAD, bf)
    out = LP.conv3x3(z.to(cuda), img, cin, addend=addend.to(cuda), mask_src=mask.to(cuda))
    ref, bnd = R.conv_model(z, R.dgrad_weight(w.to(bf)), addend=addend, mask_src=mask)
    check(out, ref, bnd, f"conv3x3 input gradient {shape} mask {mask_dt}")
    # and it IS the gradient: autograd of the fp64 forward convolution on the same operands
    zz = R.nchw(z.double())
    x0 = torch.zeros((N, cin, H, W), dtype=torch.float64, requires_grad=True)
    torch.nn.functional.conv2d(x0, w.to(bf).double(), padding=1).backward(zz)
    want = (R.nhwc(x0.grad) + addend.double()) * (mask.double() > 0)
    assert float((ref - want).abs().max()) <= 1e-12 * float(want.abs().max())


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_first_layer_forward(cuda, dt):
    x = u(7, (2, 3, 37, 50))
    w, b = conv_weight(8, 64, 3), u(9, (64,), -0.05, 0.05)
    img = LP.pack_conv(w.to(cuda), LP.PACK_FWD, dt)
    out = LP.first_forward(x.to(cuda), img, b.to(cuda), torch.tensor(R.MEAN, device=cuda), torch.tensor(R.STD, device=cuda), dt)
    ref, bnd = R.conv_model(R.first_operand(x, dt), w.to(dt), bias=b, relu=True)
    check(out, ref, bnd, f"first layer forward {dt}")


def test_first_layer_input_gradient(cuda):
    z = (u(10, (2, 37, 50, 64)) * 1e-4).to(torch.bfloat16)
    w = conv_weight(8, 64, 3)
    dx = LP.first_backward(z.to(cuda), w.to(cuda), torch.tensor(R.STD, device=cuda))
    ref, bnd = R.first_backward_model(z, w)
    assert dx.shape == (2, 3, 37, 50) and dx.dtype is torch.float32
    check(dx, ref, bnd, "first layer input gradient")


# ---- pool ------------------------------------------------------------------------------------------------------------------------------

def pool_input(dt):
    a = activation(12, (2, 9, 21, 64), dt)
    a[0, 0:2, 0:2, :] = 0.5                  # a window of four equal values: the first (row 0, column 0) wins
    a[0, 2:4, 2:4, 0:8] = torch.tensor([[0.25, 0.75], [0.75, 0.125]], dtype=dt)[:, :, None]     # a tie between positions 1 and 2: 1 wins
    a[1, 4:6, 6:8, :] = 0.0                  # an all-zero window: routed to position 0, then masked
    return a


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_maxpool_forward_is_bit_exact(cuda, dt):
    a = pool_input(dt)
    out = LP.maxpool2x2(a.to(cuda))
    pooled, _ = R.pool_route(a)
    assert out.shape == (2, 4, 10, 64) and torch.equal(out.cpu().view(torch.int16), pooled.view(torch.int16))


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_maxpool_backward(cuda, dt):
    bf = torch.bfloat16
    a = pool_input(dt)
    g = (u(13, (2, 4, 10, 64), 0.5, 1.0) * 1e-4).to(bf)          # no zero, so the routing shows in the output
    t = (u(14, (2, 9, 21, 64)) * 1e-4).to(bf)
    _, mine = R.pool_route(a)
    assert mine[0, 0, 0].all() and not mine[0, 0, 1].any() and mine[0, 2, 3, :8].all() and not mine[0, 3, 2, :8].any() and not mine[:, 8].any() \
        and not mine[:, :, 20].any()
    # routing, exactly: without a tap gradient the output is g_pooled at the first maximum of every window with a > 0, zero elsewhere
    z0 = LP.maxpool2x2_backward(a.to(cuda), g.to(cuda), torch.zeros_like(t).to(cuda)).cpu()
    gfull = torch.zeros_like(t)
    gfull[:, :8, :20] = g.repeat_interleave(2, 1).repeat_interleave(2, 2)
    want = torch.where(mine & (a.double() > 0), gfull, torch.zeros_like(gfull))
    assert torch.equal(z0.view(torch.int16), want.view(torch.int16))
    z = LP.maxpool2x2_backward(a.to(cuda), g.to(cuda), t.to(cuda))
    ref, bnd = R.pool_backward_model(a, g, t)
    check(z, ref, bnd, f"pool backward {dt}")
    assert torch.equal(z.cpu()[:, 8].double(), (t[:, 8].double() * (a[:, 8].double() > 0)))        # the dropped row: tap_grad only


# ---- taps ------------------------------------------------------------------------------------------------------------------------------

TAP_SHAPES = [(3, 5, 7, 64), (2, 9, 4, 128), (2, 3, 3, 256), (2, 2, 5, 512)]


def tap_inputs(shape, dt):
    ax, ay = activation(15, shape, dt), activation(16, shape, dt)
    ax[0, 1, 1] = 0                          # a pixel whose activations are all zero (the + 1e-10 keeps it finite)
    ay[-1, 0, 2] = 0
    lin = u(17, (shape[3],), 0.0, 2.0 / shape[3])
    return ax, ay, lin


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", TAP_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_tap_forward(cuda, shape, dt):
    ax, ay, lin = tap_inputs(shape, dt)
    out = LP.tap_forward(ax.to(cuda), ay.to(cuda), lin.to(cuda)).cpu().double()
    ref = R.tap_terms(ax, ay, lin)
    yard = float(((R.tap_terms(ax, ay, lin, torch.float32).double() - ref).abs() / ref).max())
    err = float(((out - ref).abs() / ref).max())
    print(f"tap forward {shape} {dt}: relative error {err:.2e}, torch fp32 {yard:.2e}")
    assert err <= 4 * yard
    again = LP.tap_forward(ax.to(cuda), ay.to(cuda), lin.to(cuda)).cpu().double()
    assert torch.equal(out, again)


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", TAP_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_tap_backward(cuda, shape, dt):
    ax, ay, lin = tap_inputs(shape, dt)
    up = u(18, (shape[0],), 0.2, 0.5)
    ref = R.tap_grad(ax, ay, lin, up)
    # the closed form is the derivative: autograd of the fp64 terms, away from the all-zero pixel (where torch's sqrt gives NaN)
    a = ax.double().requires_grad_(True)
    (R.tap_terms(a, ay, lin) * up.double()).sum().backward()
    ok = torch.isfinite(a.grad)
    assert int((~ok).sum()) == shape[3] and float((a.grad[ok] - ref[ok]).abs().max()) <= 1e-12 * float(ref[ok].abs().max())
    # 4 x what torch's fp32 evaluation of the same formula reaches (per pixel: its largest error over the channels), then the bf16 rounding
    yard = (R.tap_grad(ax, ay, lin, up, torch.float32).double() - ref).abs().amax(-1, keepdim=True).expand_as(ref)
    bnd = _round_bound(ref, 4 * yard, torch.bfloat16)
    out = LP.tap_backward(ax.to(cuda), ay.to(cuda), lin.to(cuda), up.to(cuda))
    assert out.dtype is torch.bfloat16
    check(out, ref, bnd, f"tap backward {shape} {dt}")
    masked = LP.tap_backward(ax.to(cuda), ay.to(cuda), lin.to(cuda), up.to(cuda), relu_mask=True).cpu()
    assert torch.equal(masked.view(torch.int16), torch.where(ax.double() > 0, out.cpu(), torch.zeros_like(masked)).view(torch.int16))
    assert float(masked[0, 1, 1].abs().max()) == 0.0 and float(out[0, 1, 1].float().abs().max()) > 0


# ---- end to end ------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def weights():
    return R.seeded_weights(SEED)


@pytest.fixture(scope="module")
def oracle(weights):
    """Per shape: inputs, the fp64 loss and gradient, and the deviation of the reference's mixed precision from them: the same torch
    composition under torch.autocast('cpu', dtype=torch.bfloat16).  Computed once for every test of this module."""
    out = {}
    for k, shape in enumerate(E2E_SHAPES):
        x, y = R.seeded_images(200 + k, shape)
        loss, grad = R.loss_and_grad(x, y, weights)
        la, ga = R.loss_and_grad(x, y, weights, dtype=torch.float32, autocast=torch.bfloat16)
        out[shape] = dict(x=x, y=y, loss=loss, grad=grad, yard_loss=float((la - loss).abs() / loss),
                          yard_grad=float((ga - grad).norm() / grad.norm()))
        print(f"oracle {shape}: loss {float(loss):.6e}, bf16 autocast deviates {out[shape]['yard_loss']:.2e} (loss) "
              f"{out[shape]['yard_grad']:.2e} (gradient, relative L2)")
    return out


def module(weights, dev, dt, chunk=None):
    m = LP.LPIPS(dtype=dt, chunk=chunk)
    m.load_state_dict(weights)
    return m.to(dev)


def run(m, x, y):
    xr = x.clone().requires_grad_(True)
    loss = m(xr, y)
    loss.backward()
    return loss.detach(), xr.grad


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_end_to_end_against_fp64(cuda, weights, oracle, dt):
    m = module(weights, cuda, dt)
    loss_bar = 2 * max(o["yard_loss"] for o in oracle.values())
    for shape, o in oracle.items():
        loss, grad = run(m, o["x"].to(cuda), o["y"].to(cuda))
        assert loss.dim() == 0 and loss.dtype is torch.float32 and grad.shape == o["x"].shape and torch.isfinite(grad).all()
        dl = float((loss.cpu().double() - o["loss"]).abs() / o["loss"])
        dg = float((grad.cpu().double() - o["grad"]).norm() / o["grad"].norm())
        print(f"LPIPS {shape} {dt}: loss deviates {dl:.2e} (bar {loss_bar:.2e}), gradient relative L2 {dg:.2e} "
              f"(yardstick {o['yard_grad']:.2e}, ratio {dg / o['yard_grad']:.2f})")
        assert dl <= loss_bar, shape
        assert dg <= 2 * o["yard_grad"], shape


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_runs_are_bit_identical_and_chunking_changes_nothing(cuda, weights, oracle, dt):
    o = oracle[E2E_SHAPES[1]]
    x, y = o["x"].to(cuda), o["y"].to(cuda)
    m = module(weights, cuda, dt)
    l1, g1 = run(m, x, y)
    l2, g2 = run(m, x, y)
    assert torch.equal(l1, l2) and torch.equal(g1, g2)
    lc, gc = run(module(weights, cuda, dt, chunk=1), x, y)
    assert torch.equal(gc, g1)
    assert abs(float(lc) - float(l1)) <= 10 * 2.0 ** -24 * float(l1)          # one fp32 rounding per added term: 5 taps x 2 images
    assert m.packed() is m.packed()                                            # packed once, not per step


def test_equal_images_give_exactly_zero(cuda, weights, oracle):
    x = oracle[E2E_SHAPES[2]]["x"].to(cuda)
    loss, grad = run(module(weights, cuda, torch.float16), x, x.clone())
    assert float(loss) == 0.0 and float(grad.abs().max()) == 0.0


def test_errors_on_the_gpu(cuda, weights):
    m = module(weights, cuda, torch.float16)
    x = torch.zeros((1, 3, 16, 16), device=cuda)
    with pytest.raises(ValueError):
        m(x, x.clone().requires_grad_(True))
    with pytest.raises(ValueError):
        m(x, torch.zeros((1, 3, 16, 17), device=cuda))
    with pytest.raises(ValueError):
        m(torch.zeros((1, 3, 15, 16), device=cuda), torch.zeros((1, 3, 15, 16), device=cuda))
    with pytest.raises(ValueError):
        m(torch.zeros((1, 1, 16, 16), device=cuda), torch.zeros((1, 1, 16, 16), device=cuda))


def test_render_loss_frames_with_lpips(cuda, weights):
    from gvfdiffusion_amd.training import render_loss_frames
    P, S, V, w = 2000, 64, 2, 0.5
    attrs = synthetic.random_gaussians(P, sh_degree=0, seed=21, scale_lo=0.01, scale_hi=0.05)
    deltas = synthetic.random_deltas(V, P, seed=22, std=0.01).to(cuda)
    ext = torch.stack([synthetic.orbit_w2c(40.0 * f + 7.0, 10.0) for f in range(V)]).to(cuda)
    K = synthetic.intrinsics().to(cuda)
    rend = GaussianRenderer({"resolution": S, "near": synthetic.NEAR, "far": synthetic.FAR, "ssaa": 1, "bg_color": (0.3, 0.3, 0.3)})
    rend.pipe.use_mip_gaussian = True
    rend.pipe.kernel_size = synthetic.KERNEL_2D
    m = module(weights, cuda, torch.float16)
    with torch.no_grad():
        gm = synthetic.gaussian_model_from(attrs, 0, cuda)
        targets = rend.render_frames(gm, ext, K, delta_pc=synthetic.random_deltas(V, P, seed=23, std=0.02).to(cuda),
                                     delta_index=list(range(V)))["rgb"].clone()
        frames = rend.render_frames(gm, ext, K, delta_pc=deltas, delta_index=list(range(V)))["rgb"]
        want = IL.image_loss(frames, targets) + w * m(frames * 2 - 1, targets * 2 - 1)
        assert float(m(frames * 2 - 1, targets * 2 - 1)) > 0
    d = deltas.clone().requires_grad_(True)
    plain = render_loss_frames(rend, gm, ext, K, d, targets)
    plain.backward()
    g_plain, d.grad = d.grad.clone(), None
    loss = render_loss_frames(rend, gm, ext, K, d, targets, lpips=m, lpips_weight=w)
    assert torch.equal(loss.detach(), want)
    loss.backward()
    assert torch.isfinite(d.grad).all() and float(d.grad.abs().max()) > 0 and not torch.equal(d.grad, g_plain)
