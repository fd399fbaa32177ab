"""Host tests of the image-loss conformance machinery (tests/ssim_ref.py: stage_a / stage_b / stage_c / judge): the measure that
tests/test_image_loss_conformance_gpu.py holds csrc/loss.hip to must bite.  No GPU.

The stand-in candidate is ssim_ref.emulate: the two stencil kernels and the reducer restated in torch fp32 on the host (separable
taps, the kernels' grouping of operations).  Unmutated it is inside every bound at every shape and input kind of the device test;
its worst err / bound over all 60 cases:
    stage A (maps a, b, c) 0.146     stage B (gradient from its own maps) 0.287     stage C (terms) 0.944
(stage C's worst is the fp32 conversion of a term against its own double sum: a rounding measured against the largest a rounding can
be, so close to 1 by construction; against float64 the two means stay under 0.2).  The reference's bound on S is at most 6.9e-5 over
all of them (const at 3 x 17 x 65), under ssim_ref.S_LEVEL everywhere.

Each mutant of the stand-in fails at its named case in the stages with a figure, and stays inside the stages marked "-" (worst
err / bound there, A / B / C; the unmutated worst at those cases is A 0.10, B 0.29, C 0.60):
    replicate  border pixels replicated into the halo, not zeros        (3, 5, 7) noise      A 2.8e5   B 8.2e5   C 7.5e3
    seam_x     contributions across the x = 64 seam dropped (halo 4)    (3, 17, 65) noise    A 1.6e3   B 1.5e3   C -
    seam_y     the same across the y = 16 seam                          (3, 17, 65) noise    A 6.2e2   B 1.4e3   C -
    plane      plane k computed from plane k - 1's pixels               (2, 11, 11) noise    A 3.9e5   B -       C -
    half_b     2p G*b written as p G*b                                  (3, 5, 7) noise      A -       B 2.5e5   C -
    sign0      sign(0) = 1                                              (2, 37, 53) ties     A -       B 8.4e6   C -
    n_hw       n = H W, not planes H W                                  (2, 11, 11) noise    A -       B 3.5e6   C 3.4e6
    no_c2      C2 missing from the numerator                            (1, 1, 1) noise      A 4.2e3   B -       C 5.4e3
    tap        the centre tap x (1 + 1e-4)                              (2, 16, 64) noise    A 27      B 53      C (1.2)
The seam mutants change no bit where there is no seam ((2, 16, 64) is one tile): asserted.  The plane mutant keeps stage B and C: it
permutes whole planes, the means do not move and stage B takes the candidate's own maps; it is stage A that sees it.  The tap mutant is
visible in A and B: 1e-4 of the centre tap is 2.7e-5 of a moment against C_M u = 1.4e-6; the means average it down to the edge of
stage C's bound (1.2), which is neither required to catch it nor to let it pass."""
import pytest
import torch

import ssim_ref as R

GTERMS = (1.25, 0.5, -0.75)            # incoming gradients of (loss, mean L1, mean SSIM): every product of coef_of is exercised
W_L1, W_SSIM = 0.8, 0.2

# mutant -> (shape, kind, the stages that must fail there, the stages that must not)
MUTANTS = {
    "replicate": ((3, 5, 7), "noise", "ABC", ""),
    "seam_x": ((3, 17, 65), "noise", "AB", "C"),
    "seam_y": ((3, 17, 65), "noise", "AB", "C"),
    "plane": ((2, 11, 11), "noise", "A", "BC"),
    "half_b": ((3, 5, 7), "noise", "B", "AC"),
    "sign0": ((2, 37, 53), "ties", "B", "AC"),
    "n_hw": ((2, 11, 11), "noise", "BC", "A"),
    "no_c2": ((1, 1, 1), "noise", "AC", "B"),
    "tap": ((2, 16, 64), "noise", "AB", ""),
}


def _judge(shape, kind, mut=()):
    p, g = R.make_inputs(kind, shape)
    out, share = R.judge(p, g, R.emulate(p, g, GTERMS, W_L1, W_SSIM, mut), GTERMS, W_L1, W_SSIM)
    print(f"{shape} {kind} {'/'.join(mut) or 'unmutated'}: " + "  ".join(f"{s} {nb} out, worst {r:.3g}" for s, (nb, r) in out.items()) +
          f"  S bound > {R.S_LEVEL:g}: {share:.3f}")
    return out, share


def test_the_mutant_table_is_the_list():
    assert set(MUTANTS) == set(R.MUTATIONS)


@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_unmutated_stand_in_is_inside_every_bound(shape):
    for kind in R.KINDS:
        out, share = _judge(shape, kind)
        assert all(nb == 0 for nb, _ in out.values()), (kind, out)
        assert share == 0.0, (kind, share)


@pytest.mark.parametrize("mut", sorted(MUTANTS))
def test_mutant_fails_its_named_case(mut):
    shape, kind, stages, keeps = MUTANTS[mut]
    base, _ = _judge(shape, kind)
    assert all(nb == 0 for nb, _ in base.values())
    out, _ = _judge(shape, kind, (mut,))
    assert all(out[s][0] > 0 for s in stages) and all(out[s][0] == 0 for s in keeps), (mut, out)
    for s in stages:
        assert out[s][1] > 10 * max(base[s][1], 1.0), (mut, s, out[s], base[s])      # well outside, not at the edge


@pytest.mark.parametrize("mut", ["seam_x", "seam_y"])
def test_seam_mutants_change_nothing_inside_one_tile(mut):
    p, g = R.make_inputs("noise", (2, 16, 64))
    a, b = R.emulate(p, g, GTERMS, W_L1, W_SSIM), R.emulate(p, g, GTERMS, W_L1, W_SSIM, (mut,))
    assert all(torch.equal(x, y) for x, y in zip(a["maps"], b["maps"])) and torch.equal(a["grad"], b["grad"])
    assert torch.equal(a["terms"], b["terms"])


def test_stage_references_agree_with_the_oracle():
    """closing() without roundings is ssim_map64 up to the window (the separable taps against their rounded outer product: 2^-24
    per weight), and stage B on the float64 maps is the autograd gradient of loss64."""
    p, g = R.make_inputs("noise", (2, 21, 69))
    ref, bnd = R.stage_a(p, g)
    assert float((ref["S"] - R.ssim_map64(p, g)[0]).abs().max()) <= 1e-5
    assert float((ref["S"] - R.ssim_map64(p, g)[0]).abs().max()) <= float(bnd["S"].max())
    x = p.double().clone().requires_grad_(True)
    m = [R.wsep64(v) for v in (x, g.double(), x * x, g.double() ** 2, x * g.double())]
    S = R.closing(m)["S"]
    (W_L1 * (x - g.double()).abs().mean() + W_SSIM * (1 - S.mean())).backward()
    n = p.numel()
    got, _ = R.stage_b(p, g, [ref[k] for k in "abc"], (1.0, 0.0, 0.0), W_L1, W_SSIM)
    k1, ks = R.coef32((1.0, 0.0, 0.0), W_L1, W_SSIM, n)
    assert abs(k1 * n - W_L1) <= 4 * R.U32 and abs(ks * n + W_SSIM) <= 4 * R.U32
    assert float((got - x.grad).abs().max()) <= 1e-6 * float(x.grad.abs().max())


def test_coef32_rounds_as_fp32():
    n = 3 * 33 * 129
    k1, ks = R.coef32(GTERMS, W_L1, W_SSIM, n)
    f = lambda v: torch.tensor(v, dtype=torch.float32)  # noqa: E731
    inv = f(1.0) / f(float(n))
    assert k1 == float((f(1.25) * f(0.8) + f(0.5)) * inv) and ks == float((f(-0.75) - f(1.25) * f(0.2)) * inv)
    assert k1 == float(f(k1)) and ks == float(f(ks))                      # both are fp32 values
    assert abs(k1 - (1.25 * 0.8 + 0.5) / n) <= 4 * R.U32 * abs(k1)
