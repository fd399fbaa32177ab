"""The host reference of the sparse-convolution family (tests/spconv_ref.py) is checked on the CPU before the kernels are measured by it:
reference() against float64 F.conv3d on the densified grid, and bound() against mutants -- outputs of a convolution that is wrong in one
of the ways this operator can be wrong -- each of which it must reject, while the correctly rounded output passes."""
import pytest
import torch

import spconv_ref as S

DTS = [torch.bfloat16, torch.float16]


@pytest.fixture(scope="module")
def case():
    coords = S.standard_coords(permuted=True)
    x16, w16, _, bias, addend = S.make_operands(coords.shape[0], 64, 64, torch.bfloat16, seed=1)
    nbr = S.neighbor_map(coords)
    return coords, nbr, x16, w16, bias, addend


def test_standard_input_is_what_the_family_says():
    c = S.standard_coords()
    assert c.shape == (1192, 4) and int((c[:, 0] == 0).sum()) == 552 and int((c[:, 0] == 1).sum()) == 640
    n = (S.neighbor_map(c) >= 0).sum(1)
    assert int(n.min()) >= 12 and int(n.max()) == 27
    assert len({tuple(r) for r in c.tolist()}) == 1192
    assert S.shell(64, 24, 26).shape[0] == 15968
    for name, e in S.edge_sets().items():
        assert len({tuple(r) for r in e.tolist()}) == e.shape[0], name
    assert int((S.neighbor_map(S.edge_sets()["checker"]) >= 0).sum(1).max()) == 1


@pytest.mark.parametrize("dt", DTS, ids=["bf16", "fp16"])
def test_reference_is_the_dense_convolution(dt):
    """The neighbour-map form equals conv3d(dense, W.permute(0,4,1,2,3), padding=1) at the active sites: cross-correlation, kernel axes in
    coordinate-column order, samples apart."""
    for coords in (S.standard_coords(permuted=True), S.edge_sets()["twins"], S.edge_sets()["solid6"]):
        x16, w16, _, bias, _ = S.make_operands(coords.shape[0], 64, 64, dt, seed=3)
        ref = S.reference(x16, S.neighbor_map(coords), w16, bias)
        dense = S.dense_conv3d(x16, coords, w16, bias)
        assert float((ref - dense).abs().max()) <= 1e-12


def _outside(out, ref, bnd):
    return S.excess(out, ref, bnd)[0]


def test_correct_outputs_pass(case):
    coords, nbr, x16, w16, bias, addend = case
    for kw in (dict(), dict(bias=bias), dict(bias=bias, addend=addend)):
        ref, bnd = S.model(x16, nbr, w16, **kw)
        assert _outside(ref.float(), ref, bnd) == 0
        ref, bnd = S.model(x16, nbr, w16, out_dt=torch.bfloat16, **kw)
        assert _outside(ref.float().to(torch.bfloat16), ref, bnd) == 0


def test_bound_rejects_wrong_convolutions(case):
    coords, nbr, x16, w16, bias, addend = case
    ref, bnd = S.model(x16, nbr, w16, bias)
    mutants = {
        "flipped taps": S.reference(x16, nbr.flip(1), w16, bias),
        "x and z swapped": S.reference(x16, nbr, w16.permute(0, 3, 2, 1, 4).contiguous(), bias),
        "dropped bias": S.reference(x16, nbr, w16, None),
    }
    one = nbr.clone()
    row = int(torch.nonzero(one[:, 5] >= 0)[0])
    one[row, 5] = -1
    mutants["one missing tap on one row"] = S.reference(x16, one, w16, bias)
    for name, out in mutants.items():
        assert _outside(out.float(), ref, bnd) > 0, name
    assert _outside(mutants["one missing tap on one row"].float(), ref, bnd) == 64        # that row's outputs, nothing else


def test_bound_rejects_wrong_maps():
    sets = S.edge_sets()
    for name, kw in (("faces", dict(wrap10=True)), ("twins", dict(cross_sample=True))):
        coords = sets[name]
        x16, w16, _, bias, _ = S.make_operands(coords.shape[0], 64, 64, torch.float16, seed=5)
        good, bad = S.neighbor_map(coords), S.neighbor_map(coords, **kw)
        assert not torch.equal(good, bad), name
        ref, bnd = S.model(x16, good, w16, bias)
        assert _outside(S.reference(x16, bad, w16, bias).float(), ref, bnd) > 0, name


@pytest.mark.parametrize("dt", DTS, ids=["bf16", "fp16"])
def test_bound_rejects_a_truncating_store(case, dt):
    coords, nbr, x16, w16, bias, addend = case
    x16, w16 = x16.to(dt), w16.to(dt)
    ref, bnd = S.model(x16, nbr, w16, bias, addend, out_dt=dt)
    nearest = ref.float().to(dt)
    assert _outside(nearest, ref, bnd) == 0
    # toward zero: where the nearest value is the larger neighbour, one step down in the sign-magnitude bit pattern
    up = nearest.double().abs() > ref.abs()
    bits = nearest.view(torch.int16).to(torch.int32) & 0xffff
    bits = torch.where(up, (bits & 0x8000) | ((bits & 0x7fff) - 1), bits)
    trunc = torch.where(bits >= 0x8000, bits - 0x10000, bits).to(torch.int16).view(dt)
    assert _outside(trunc, ref, bnd) > ref.numel() // 8


def test_ln_act_bound_rejects_a_missing_activation_and_a_missing_modulation():
    g = torch.Generator().manual_seed(2)
    X = torch.randn((9, 128), generator=g) * 2 + 0.3
    lw, lb = 1 + 0.1 * torch.randn(128, generator=g), 0.1 * torch.randn(128, generator=g)
    sh, sc = 0.3 * torch.randn(128, generator=g), 0.3 * torch.randn(128, generator=g)
    dt = torch.bfloat16
    ref, bnd = S.ln_act_model(X, dt, 1e-6, lw, lb, sh, sc, act=1)
    assert _outside(ref.to(dt), ref, bnd) == 0
    assert _outside(S.ln_act_model(X, dt, 1e-6, lw, lb, sh, sc, act=0)[0].to(dt), ref, bnd) > 0
    assert _outside(S.ln_act_model(X, dt, 1e-6, lw, lb, None, None, act=1)[0].to(dt), ref, bnd) > 0
    mean, var = X.double().mean(1, keepdim=True), X.double().var(1, unbiased=False, keepdim=True)
    y = ((X.double() - mean) / torch.sqrt(var + 1e-6) * lw + lb) * (1 + sc) + sh
    assert float((S.r16(y * torch.sigmoid(y), dt) - ref).abs().max()) == 0.0
