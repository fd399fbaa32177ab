"""The fused L1 + SSIM image loss (csrc/loss.hip: image_loss_fwd_kernel<GRAD>, image_loss_bwd_kernel, image_loss_bwd_l1_kernel, the
reducer) on an MI355X, element by element against the stage-wise float64 references and counted bounds of tests/ssim_ref.py (its
docstring derives them; tests/test_image_loss_conformance_ref.py shows that they bite).  The C entry points are called through ctypes
on buffers of the test's own:
  * pred and gt are views between NaN planes of a larger buffer (a read outside the planes shows), the scratch is NaN before the
    forward (a map slot read before it is written shows), sentinel rows guard the gradient and sentinel words the scratch's end;
  * the maps are the last 12 n bytes of the scratch (grad size = no-grad size + 12 n is asserted), the per-workgroup double partials
    its first 16 bytes per 64 x 16 tile;
  * stage A: the saved maps a, b, c; stage B: the gradient against the float64 window over the device's OWN maps; stage C: mean L1
    and mean SSIM against float64, each fp32 term one rounding from the device's double sum, the loss one rounding from
    w_l1 L1 + w_ssim (1 - SSIM) of those sums;
  * the terms with and without GVF_IMAGE_LOSS_SSIM_GRAD are the same bits; everything is the same bits on a second launch and on a
    side stream.
Shapes (planes, H, W) are the smallest at which each mechanism exists: widths 63 / 64 / 65 / 69 / 70 / 129 and heights 15 / 16 / 17 /
21 / 22 / 33 straddle the 64 x 16 tile, the four rows of a thread and the reach of the 5-pixel halo; planes differ in content.
Where the bound is loose (flat images) exact properties stand in: identical images, all-black pairs, zero maps, the L1-only backward.

Measured on the MI355X, worst err / bound over the 60 cases of test_stages:
    stage A 0.146 ((3, 33, 129) spikes)     stage B 0.287 ((2, 16, 64) noise)     stage C 0.944 ((3, 17, 65) spikes)
-- the figures of the host stand-in to the digit (ssim_ref.emulate restates the kernels' operations one by one).  Stage C's worst is
the fp32 conversion of a term against its own double sum, a rounding measured against the largest a rounding can be; against float64
the stand-in's two means stay under 0.19 of their bound.  Identical images: max |-2b/c - 1| = 2.00 u, |ssim - 1| = 0.
The share of pixels whose bound on S exceeds 1e-4 is 0 in every case (the largest bound is 6.9e-5, const at 3 x 17 x 65).
The whole file: 68 tests in under 3 s."""
import ctypes

import pytest
import torch

import ssim_ref as R
from gvfdiffusion_amd import _lib
from gvfdiffusion_amd.ops import image_loss as IL

pytestmark = pytest.mark.gpu
GTERMS = (1.25, 0.5, -0.75)            # incoming gradients of (loss, mean L1, mean SSIM): every product of coef_of is exercised
W_L1, W_SSIM = 0.8, 0.2
GUARD = 3                              # sentinel rows on both sides of the gradient
SENT = 12345.0
TAIL = 64                              # NaN words after the scratch's reported size


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _bytes(P, H, W, flags):
    nb = ctypes.c_size_t(0)
    assert _lib.lib().gvf_image_loss_scratch_bytes(P, H, W, flags, ctypes.byref(nb)) == _lib.GVF_OK
    assert nb.value % 4 == 0
    return int(nb.value)


def _between_nan_planes(x, dev):
    buf = torch.full((x.shape[0] + 2,) + tuple(x.shape[1:]), float("nan"), device=dev)
    buf[1:-1] = x.to(dev)
    return buf, buf[1:-1]


def _nan_words(nbytes, dev):
    return torch.full((nbytes // 4 + TAIL,), float("nan"), device=dev)


def _guarded_grad(P, H, W, dev):
    buf = torch.full((P * H + 2 * GUARD, W), SENT, device=dev)
    return buf, buf[GUARD:GUARD + P * H].view(P, H, W)


def _bits(t):
    return t.contiguous().view(torch.int32)


class Run:
    """buffers of one case and the three launches on them"""

    def __init__(self, dev, p, g, gterms=GTERMS):
        self.P, self.H, self.W = P, H, W = tuple(p.shape)
        self.n = n = P * H * W
        self.nblk = P * ((W + R.TILE_W - 1) // R.TILE_W) * ((H + R.TILE_H - 1) // R.TILE_H)
        self.nb0, self.nb1 = _bytes(P, H, W, 0), _bytes(P, H, W, IL.SSIM_GRAD)
        assert self.nb1 == self.nb0 + 12 * n and 16 * self.nblk <= self.nb0 < 16 * self.nblk + 256      # the layout this test mirrors
        self.pbuf, self.p = _between_nan_planes(p, dev)
        self.gbuf, self.g = _between_nan_planes(g, dev)
        self.sc0, self.sc1 = _nan_words(self.nb0, dev), _nan_words(self.nb1, dev)
        self.terms0, self.terms1 = (torch.full((3,), float("nan"), device=dev) for _ in range(2))
        self.gradbuf, self.grad = _guarded_grad(P, H, W, dev)
        self.gt3 = torch.tensor(gterms, dtype=torch.float32, device=dev)

    def forward(self, sp, flags):
        sc, nb, terms = (self.sc1, self.nb1, self.terms1) if flags else (self.sc0, self.nb0, self.terms0)
        _lib.check(_lib.lib().gvf_image_loss_forward(_p(self.p), _p(self.g), self.P, self.H, self.W, W_L1, W_SSIM, _p(terms), _p(sc), nb,
                                                     flags, sp), "forward")

    def backward(self, sp, flags=IL.SSIM_GRAD):
        sc, nb = (self.sc1, self.nb1) if flags else (None, 0)
        _lib.check(_lib.lib().gvf_image_loss_backward(_p(self.p), _p(self.g), self.P, self.H, self.W, W_L1, W_SSIM, _p(self.gt3),
                                                      _p(self.grad), _p(sc), nb, flags, sp), "backward")

    def all(self, stream):
        sp = ctypes.c_void_p(stream.cuda_stream)
        self.forward(sp, IL.SSIM_GRAD)
        self.forward(sp, 0)
        self.backward(sp)

    def maps(self):
        return self.sc1[self.nb1 // 4 - 3 * self.n:self.nb1 // 4].view(3, self.P, self.H, self.W)

    def means(self):
        """the double means behind terms[1], terms[2]: the per-workgroup partials (sum S, sum |p - g|), summed here"""
        part = self.sc1[:4 * self.nblk].view(torch.float64).view(self.nblk, 2).cpu()
        return float(part[:, 1].sum()) / self.n, float(part[:, 0].sum()) / self.n

    def guards_intact(self):
        g = torch.cat([self.gradbuf[:GUARD], self.gradbuf[GUARD + self.P * self.H:]])
        tails = torch.cat([self.sc0[self.nb0 // 4:], self.sc1[self.nb1 // 4:]])
        nan = _bits(torch.full((1,), float("nan")))[0].item()
        planes = torch.cat([self.pbuf[0], self.pbuf[-1], self.gbuf[0], self.gbuf[-1]])
        return bool((g == SENT).all()) and bool((_bits(tails) == nan).all()) and bool(torch.isnan(planes).all())


def _twice_and_other_stream(launch, bufs):
    """launch(stream) three times: current stream, again, and a side stream; every buffer must hold the same bits each time."""
    cur = torch.cuda.current_stream()
    launch(cur)
    torch.cuda.synchronize()
    first = [_bits(b).clone() for b in bufs]
    launch(cur)
    torch.cuda.synchronize()
    for b, f in zip(bufs, first):
        assert torch.equal(_bits(b), f), "a second launch gave other bits"
    side = torch.cuda.Stream()
    side.wait_stream(cur)
    with torch.cuda.stream(side):
        launch(side)
    side.synchronize()
    for b, f in zip(bufs, first):
        assert torch.equal(_bits(b), f), "another stream gave other bits"


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_stages(cuda, shape, kind):
    p, g = R.make_inputs(kind, shape)
    run = Run(cuda, p, g)
    _twice_and_other_stream(run.all, [run.terms0, run.terms1, run.sc0, run.sc1, run.gradbuf])
    assert run.guards_intact()
    assert torch.equal(_bits(run.terms0), _bits(run.terms1)), "the terms depend on GVF_IMAGE_LOSS_SSIM_GRAD"
    ml, ms = run.means()
    cand = dict(maps=tuple(run.maps().cpu()), grad=run.grad.cpu(), terms=run.terms1.cpu(), ml=ml, ms=ms)
    out, share = R.judge(p, g, cand, GTERMS, W_L1, W_SSIM)
    print(f"{shape} {kind}: " + "  ".join(f"{s} {nb} out, worst {r:.3g}" for s, (nb, r) in out.items()) +
          f"  S bound > {R.S_LEVEL:g}: {share:.3f}")
    assert share == 0.0, f"the reference's bound on S exceeds {R.S_LEVEL:g} on {share:.3%} of the pixels"
    assert all(nb == 0 for nb, _ in out.values()), out


def test_identical_images_give_s_of_one(cuda):
    """A1 = B1 and A2 = B2 bit for bit (-ffp-contract=off), so S is D / D: 1 to within the rounding of one division, at most one ulp
    above 1 (2 u).  Per pixel through the maps: with A1 = B1, -2 b / c = S B1 B2 / D, three more roundings (b's and c's divisions,
    D's product): |-2 b / c - 1| <= 5 u.  Through the mean: the four-term fp32 sums (3 u) and the conversion (u): 6 u."""
    for shape in [(3, 17, 65), (2, 37, 53), (2, 1, 70)]:
        p, _ = R.make_inputs("noise", shape)
        run = Run(cuda, p, p.clone())
        run.all(torch.cuda.current_stream())
        torch.cuda.synchronize()
        _, b, c = run.maps().double().cpu()
        worst = float((-2 * b / c - 1).abs().max())
        t = run.terms1.double().cpu()
        print(f"{shape} identical: max |-2b/c - 1| {worst / R.U32:.2f} u, |ssim - 1| {abs(float(t[2]) - 1) / R.U32:.2f} u")
        assert worst <= R.rounds(5) and abs(float(t[2]) - 1.0) <= R.rounds(6)
        assert float(t[1]) == 0.0
        ml, ms = run.means()
        v, bar = R.loss_of_sums(ml, ms, W_L1, W_SSIM)
        assert ml == 0.0 and abs(float(t[0]) - v) <= bar
        assert run.guards_intact()


def test_all_black_pairs(cuda):
    """Every moment is 0: S = (C1 C2) / (C1 C2) with the same rounded product on both sides, a = 0 and sign(0) = 0."""
    for shape in [(3, 17, 65), (1, 1, 1), (2, 22, 70)]:
        z = torch.zeros(shape)
        run = Run(cuda, z, z.clone())
        run.all(torch.cuda.current_stream())
        torch.cuda.synchronize()
        t = run.terms1.cpu()
        assert float(t[2]) == 1.0 and float(t[1]) == 0.0 and float(t[0]) == 0.0
        assert bool((run.grad == 0).all()) and run.guards_intact()


def test_backward_on_zero_maps_is_the_l1_gradient(cuda):
    """Only the backward entry point, on a scratch the test wrote: a = b = c = 0 (the partials stay NaN: the backward does not read them)."""
    shape = (3, 17, 65)
    p, g = R.make_inputs("ties", shape)
    run = Run(cuda, p, g)
    run.maps().zero_()
    run.backward(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    k1, _ = R.coef32(GTERMS, W_L1, W_SSIM, p.numel())
    want = torch.tensor(k1, dtype=torch.float32) * torch.sign(p - g)
    assert int((want == 0).sum()) >= 4 * 65 and torch.equal(run.grad.cpu(), want)            # value equality: -0 is 0
    assert run.guards_intact()


@pytest.mark.parametrize("n", [1, 255, 256, 257, 8192 * 256 + 257])
def test_l1_only_backward(cuda, n):
    """flag 0: image_loss_bwd_l1_kernel, 256 elements per workgroup and at most 8192 workgroups (the last n wraps the grid-stride loop);
    no scratch.  k_l1 sign(p - g) is one exact product."""
    gen = torch.Generator().manual_seed(n)
    p = torch.rand((1, 1, n), generator=gen)
    g = (p + 0.15 * torch.randn((1, 1, n), generator=gen)).clamp(0, 1)
    g[..., ::3] = p[..., ::3]
    run = Run(cuda, p, g)
    _twice_and_other_stream(lambda s: run.backward(ctypes.c_void_p(s.cuda_stream), 0), [run.gradbuf])
    k1, _ = R.coef32(GTERMS, W_L1, W_SSIM, n)
    want = torch.tensor(k1, dtype=torch.float32) * torch.sign(p - g)
    assert torch.equal(run.grad.cpu(), want) and run.guards_intact()
