"""The host reference of the dense-convolution family (tests/conv3d_ref.py) is checked on the CPU before the kernels are measured by it:
model() against float64 F.conv3d, the pixel-shuffle against the reshape form of the reference's pixel_shuffle_3d, the occupancy against
torch.argwhere, and bound() against mutants -- outputs of a convolution that is wrong in one of the ways this operator can be wrong -- each
of which it must reject, while the correctly rounded output passes."""
import pytest
import torch
import torch.nn.functional as F

import conv3d_ref as C

DTS = [torch.bfloat16, torch.float16]
GRID = (2, 5, 6, 7)


@pytest.fixture(scope="module")
def case():
    x16, w16, _, bias, addend = C.make_operands(GRID, 32, 16, torch.bfloat16, seed=1)
    return x16, w16, bias, addend


def _outside(out, ref, bnd):
    return C.excess(out, ref, bnd)[0]


def _pixel_shuffle_3d(x, s=2):
    """The dense form: [B, C, X, Y, Z] -> [B, C / s^3, sX, sY, sZ]."""
    B, Cc, X, Y, Z = x.shape
    v = x.reshape(B, Cc // s ** 3, s, s, s, X, Y, Z).permute(0, 1, 5, 2, 6, 3, 7, 4)
    return v.reshape(B, Cc // s ** 3, X * s, Y * s, Z * s)


@pytest.mark.parametrize("dt", DTS, ids=["bf16", "fp16"])
@pytest.mark.parametrize("grid,cin,cout", [(GRID, 8, 16), ((1, 1, 1, 1), 8, 1), ((1, 3, 3, 3), 40, 24), ((2, 4, 4, 4), 32, 8)])
def test_reference_is_f_conv3d(dt, grid, cin, cout):
    x16, w16, _, bias, _ = C.make_operands(grid, cin, cout, dt, seed=3, pad=8)
    ref = C.reference(x16, grid, w16, bias)
    dense = F.conv3d(C.to_dense(x16[:, :cin].double(), grid), w16.double(), bias.double(), padding=1)
    assert float((ref - C.to_rows(dense)).abs().max()) <= 1e-12
    assert torch.equal(C.to_rows(C.to_dense(x16[:, :cin], grid)), x16[:, :cin])
    if cout % 8 == 0:
        shuf = C.reference(x16, grid, w16, bias, store="shuffle2")
        assert float((shuf - C.to_rows(_pixel_shuffle_3d(dense))).abs().max()) <= 1e-12


def test_occupancy_is_argwhere():
    for grid in (GRID, (1, 1, 1, 1), (2, 3, 1, 4)):
        logits = C.make_logits(grid, seed=5)
        dense = logits.reshape(grid[0], 1, *grid[1:])
        want = torch.argwhere(dense > 0)[:, [0, 2, 3, 4]].int()
        got = C.occupancy(logits, grid)
        assert got.dtype == torch.int32 and torch.equal(got, want)
    logits = C.make_logits(GRID, seed=5)
    assert bool((logits == 0).any()) and bool(torch.isnan(logits).any()) and bool(torch.signbit(logits[logits == 0]).any())
    assert C.occupancy(logits, GRID, mutant=True).shape[0] > C.occupancy(logits, GRID).shape[0]        # `>= 0` takes the zeros in
    assert C.occupancy(torch.full((2, 210), -1.0), GRID).shape == (0, 4)
    assert C.occupancy(torch.full((2, 210), 1.0), GRID).shape == (420, 4)


def test_correct_outputs_pass(case):
    x16, w16, bias, addend = case
    for kw in (dict(), dict(bias=bias), dict(bias=bias, addend=addend)):
        ref, bnd = C.model(x16, GRID, w16, **kw)
        assert _outside(ref.float(), ref, bnd) == 0
        ref, bnd = C.model(x16, GRID, w16, out_dt=torch.bfloat16, **kw)
        assert _outside(ref.float().to(torch.bfloat16), ref, bnd) == 0
    ref, bnd = C.model(x16, GRID, w16, bias, store="shuffle2")
    assert ref.shape == (8 * x16.shape[0], 2) and _outside(ref.float(), ref, bnd) == 0


def test_bound_rejects_wrong_convolutions(case):
    x16, w16, bias, addend = case
    ref, bnd = C.model(x16, GRID, w16, bias)
    mutants = {
        "flipped taps": C.reference(x16, GRID, w16, bias, flip=True),
        "periodic padding": C.reference(x16, GRID, w16, bias, mutant="periodic"),
        "row +- 1 across boundaries": C.reference(x16, GRID, w16, bias, mutant="rowshift"),
        "x and z swapped": C.reference(x16, GRID, w16.permute(0, 1, 4, 3, 2).contiguous(), bias),
        "dropped bias": C.reference(x16, GRID, w16, None),
    }
    for name, out in mutants.items():
        assert _outside(out.float(), ref, bnd) > 0, name
    # periodic padding and the flat row shift are wrong at the faces only: the interior voxels pass
    B, X, Y, Z = GRID
    inner = torch.zeros((B, X, Y, Z), dtype=torch.bool)
    inner[:, 1:-1, 1:-1, 1:-1] = True
    inner = inner.reshape(-1)
    for name in ("periodic padding", "row +- 1 across boundaries"):
        out = mutants[name].float()
        assert _outside(out[inner], ref[inner], bnd[inner]) == 0, name
    wrong = lambda name: ((mutants[name].double() - ref).abs() > bnd).any(1).reshape(B, X, Y, Z)
    assert bool(wrong("periodic padding").reshape(-1)[~inner].all())                # every face voxel is wrong somewhere
    # the flat row shift: a z face, a y face and the first x layer of sample 1 (whose x - 1 neighbours are sample 0's last layer); the
    # first x layer of sample 0 is right by accident (those rows do not exist)
    w = wrong("row +- 1 across boundaries")
    assert bool(w[0, 2, 2, 0]) and bool(w[0, 2, 2, Z - 1]) and bool(w[0, 2, 0, 3]) and bool(w[0, 2, Y - 1, 3]) and bool(w[1, 0, 2, 3])
    assert not bool(w[0, 0, 2, 3])


def test_bound_rejects_a_reversed_pixel_shuffle(case):
    x16, w16, bias, _ = case
    ref, bnd = C.model(x16, GRID, w16, bias, store="shuffle2")
    rows = C.reference(x16, GRID, w16, bias)
    assert _outside(C.pixel_shuffle2(rows, GRID).float(), ref, bnd) == 0
    assert _outside(C.pixel_shuffle2(rows, GRID, reversed_ijk=True).float(), ref, bnd) > ref.numel() // 4


@pytest.mark.parametrize("dt", DTS, ids=["bf16", "fp16"])
def test_bound_rejects_a_truncating_store(case, dt):
    x16, w16, bias, addend = case
    x16, w16 = x16.to(dt), w16.to(dt)
    ref, bnd = C.model(x16, GRID, w16, bias, addend, out_dt=dt)
    nearest = ref.float().to(dt)
    assert _outside(nearest, ref, bnd) == 0
    # toward zero: where the nearest value is the larger neighbour, one step down in the sign-magnitude bit pattern
    up = nearest.double().abs() > ref.abs()
    bits = nearest.view(torch.int16).to(torch.int32) & 0xffff
    bits = torch.where(up, (bits & 0x8000) | ((bits & 0x7fff) - 1), bits)
    trunc = torch.where(bits >= 0x8000, bits - 0x10000, bits).to(torch.int16).view(dt)
    assert _outside(trunc, ref, bnd) > ref.numel() // 8
