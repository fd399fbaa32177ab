"""Element-wise conformance of the submanifold sparse 3x3x3 convolution family (csrc/spconv.hip; include/gvf_spconv.h) against the host
reference and bound of tests/spconv_ref.py (which tests/test_spconv_ref.py checks on the CPU): the neighbour map exactly, every output of
the convolution within bound(), the LayerNorm + activation link within the bar of tests/test_elem_conformance_gpu.py.  Standard input:
shell(16, 4.5, 6.0) in sample 0 and shell(16, 2.0, 5.5) in sample 1 -- 1192 rows, 18.6 tiles of 64, 12 to 27 neighbours per row -- in grid
order and in a seeded random permutation."""
import pytest
import torch

import spconv_ref as S
from gvfdiffusion_amd.ops import spconv

pytestmark = pytest.mark.gpu
DTYPES = [torch.bfloat16, torch.float16]
SENTINEL16 = 0x7E5A
GUARD = 3


@pytest.fixture(scope="module")
def maps():
    """name -> (coords, dict-built map): computed once, shared, never modified."""
    out = {"grid": S.standard_coords(False), "perm": S.standard_coords(True)}
    out.update(S.edge_sets())
    return {k: (c, S.neighbor_map(c)) for k, c in out.items()}


@pytest.mark.parametrize("name", ["grid", "perm", "one", "t63", "t64", "t65", "solid6", "checker", "faces", "twins"])
def test_neighbor_map_is_exact(cuda, maps, name):
    coords, want = maps[name]
    got = spconv.build_neighbor_map(coords.to(cuda))
    again = spconv.build_neighbor_map(coords.to(cuda))
    assert got.dtype == torch.int32 and tuple(got.shape) == (coords.shape[0], 27)
    assert torch.equal(got.cpu(), want), f"{name}: {int((got.cpu() != want).sum())} entries differ"
    assert torch.equal(got, again)
    if name == "checker":
        assert int((want >= 0).sum(1).max()) == 1
    if name == "twins":
        half = coords.shape[0] // 2
        assert int(want[:half].max()) < half and int(want[half:][want[half:] >= 0].min()) >= half


def test_neighbor_map_ignores_rows_outside_the_grid(cuda):
    """A row whose coordinates are not in [0, 1024) is in nobody's neighbourhood and has no neighbours (it is not packed into a key)."""
    c = torch.tensor([[0, 1023, 5, 5], [0, 1024, 5, 5], [0, 0, 5, 5], [0, -1, 5, 5], [0, 1022, 5, 5]], dtype=torch.int32)
    got = spconv.build_neighbor_map(c.to(cuda)).cpu()
    want = torch.full((5, 27), -1, dtype=torch.int32)
    want[0, 13], want[2, 13], want[4, 13], want[0, 4], want[4, 22] = 0, 2, 4, 4, 0
    assert torch.equal(got, want)


def _run(cuda, dt, coords, nbr, cin, cout, out_dt, with_bias, with_addend, ld_in, seed):
    """-> (device output [T, cout], reference, bound, device inputs)."""
    T = coords.shape[0]
    x16, w16, w32, bias, addend = S.make_operands(T, cin, cout, dt, seed, ld_in)
    bias = bias if with_bias else None
    addend = addend if with_addend else None
    ref, bnd = S.model(x16, nbr, w16, bias, addend, None if out_dt is torch.float32 else dt)
    # rows beyond T: NaN operand rows that no map entry names, a sentinel in the output buffer
    xbuf = torch.full((T + GUARD, x16.shape[1]), float("nan"), dtype=dt, device=cuda)
    xbuf[:T] = x16.to(cuda)
    wimg = spconv.pack_weight(w32.to(cuda), dt)
    dev = lambda t: None if t is None else t.to(cuda)
    if out_dt is torch.float32:
        obuf = torch.full((T + 2 * GUARD, cout), float("nan"), dtype=torch.float32, device=cuda)
    else:
        obuf = torch.full((T + 2 * GUARD, cout), SENTINEL16, dtype=torch.int16, device=cuda).view(dt)
    args = (xbuf[:T], nbr.to(cuda), wimg, cout)
    kw = dict(bias=dev(bias), addend=dev(addend), out_dtype=out_dt, cin=cin, out=obuf[GUARD:GUARD + T])
    spconv.conv3(*args, **kw)
    torch.cuda.synchronize()
    return obuf, ref, bnd, args, kw


def _check(obuf, ref, bnd, T, what):
    out = obuf[GUARD:GUARD + T].cpu()
    guard = torch.cat([obuf[:GUARD], obuf[GUARD + T:]]).cpu()
    if obuf.dtype is torch.float32:
        assert bool(torch.isnan(guard).all()), "a store outside the rows of the call"
    else:
        assert bool((guard.view(torch.int16) == SENTINEL16).all()), "a store outside the rows of the call"
    assert torch.isfinite(out.float()).all(), f"{what}: a padding column or a row beyond T was read"
    n_bad, worst = S.excess(out, ref, bnd)
    print(f"spconv {what}: worst |err| / bound {worst:.3f}")
    assert n_bad == 0, f"{what}: {n_bad} of {out.numel()} elements outside the bound (worst {worst:.3g} x)"


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("out32", [True, False], ids=["f32out", "lpout"])
@pytest.mark.parametrize("cin,cout,order,with_bias,with_addend,pad", [
    (64, 64, "perm", True, True, 8), (64, 64, "grid", False, False, 0), (64, 128, "perm", True, False, 0), (64, 128, "grid", False, True, 24),
    (256, 64, "perm", True, True, 0), (256, 64, "grid", False, False, 64), (128, 128, "perm", False, True, 0), (128, 128, "grid", True, False, 8),
    (64, 256, "perm", True, True, 0)])
def test_conv_every_element_within_bound(cuda, maps, dt, out32, cin, cout, order, with_bias, with_addend, pad):
    coords, nbr = maps[order]
    out_dt = torch.float32 if out32 else dt
    obuf, ref, bnd, _, _ = _run(cuda, dt, coords, nbr, cin, cout, out_dt, with_bias, with_addend, cin + pad, seed=cin + cout)
    _check(obuf, ref, bnd, coords.shape[0], f"{cin}->{cout} T{coords.shape[0]} {order} bias{int(with_bias)} add{int(with_addend)} ld+{pad} {dt} -> {out_dt}")


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("out32", [True, False], ids=["f32out", "lpout"])
def test_conv_deep_contraction(cuda, maps, dt, out32):
    """(1024, 64) at T = 200: 27 x 32 k-steps; the first 200 rows of the permuted standard input (neighbours beyond them are absent)."""
    coords = maps["perm"][0][:200].contiguous()
    nbr = S.neighbor_map(coords)
    out_dt = torch.float32 if out32 else dt
    obuf, ref, bnd, _, _ = _run(cuda, dt, coords, nbr, 1024, 64, out_dt, True, True, 1024 + 8, seed=11)
    _check(obuf, ref, bnd, 200, f"1024->64 T200 {dt} -> {out_dt}")


@pytest.mark.parametrize("name", ["one", "t63", "t64", "t65", "checker", "faces", "twins"])
def test_conv_on_the_edge_sets(cuda, maps, name):
    coords, nbr = maps[name]
    dt = torch.float16
    obuf, ref, bnd, _, _ = _run(cuda, dt, coords, nbr, 64, 64, torch.float32, True, False, 64, seed=len(name))
    _check(obuf, ref, bnd, coords.shape[0], f"64->64 {name}")


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
def test_nan_row_poisons_exactly_its_neighbourhood(cuda, maps, dt):
    coords, nbr = maps["perm"]
    T, cin, cout = coords.shape[0], 64, 128
    x16, w16, w32, bias, _ = S.make_operands(T, cin, cout, dt, seed=21)
    bad = 777
    x16[bad] = float("nan")
    out = spconv.conv3(x16.to(cuda), nbr.to(cuda), spconv.pack_weight(w32.to(cuda), dt), cout, bias=bias.to(cuda)).cpu()
    lists_it = (nbr == bad).any(1)
    assert 12 <= int(lists_it.sum()) <= 27
    assert bool(torch.isnan(out[lists_it]).all()), "a row that lists the NaN row as a neighbour has finite outputs"
    assert bool(torch.isfinite(out[~lists_it]).all()), "the NaN row reached a row that does not list it"
    x16[bad] = 0
    ref, bnd = S.model(x16, nbr, w16, bias)
    assert S.excess(out[~lists_it], ref[~lists_it], bnd[~lists_it])[0] == 0


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
def test_equal_bits_twice_and_on_two_streams(cuda, maps, dt):
    coords, nbr = maps["perm"]
    obuf, _, _, args, kw = _run(cuda, dt, coords, nbr, 128, 128, torch.float32, True, True, 128, seed=31)
    first = obuf.clone()
    spconv.conv3(*args, **kw)
    torch.cuda.synchronize()
    assert torch.equal(obuf.view(torch.int32), first.view(torch.int32)), "a second launch gave other bits"
    outs = [torch.empty_like(kw["out"]) for _ in range(2)]
    streams = [torch.cuda.Stream(device=cuda) for _ in range(2)]
    torch.cuda.synchronize()
    for _ in range(3):
        for s, o in zip(streams, outs):
            with torch.cuda.stream(s):
                spconv.conv3(*args, **dict(kw, out=o))
    torch.cuda.synchronize()
    want = first[GUARD:GUARD + coords.shape[0]].view(torch.int32)
    assert all(torch.equal(o.view(torch.int32), want) for o in outs), "two streams gave other bits"


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("act", [0, 1], ids=["id", "silu"])
@pytest.mark.parametrize("mode", ["plain", "affine", "adaln", "both"])
@pytest.mark.parametrize("C,rows", [(64, 37), (128, 130), (1024, 41), (2048, 5), (100, 6)])
def test_ln_act_elementwise(cuda, dt, act, mode, C, rows):
    g = torch.Generator().manual_seed(C + rows + act)
    x = torch.randn((rows, C), generator=g) * 2 + 0.5
    x[0:2] += 200.0                                               # |mean| = 100 x std
    x[2] = 3.0                                                    # variance 0: eps decides
    x[3, 1::29] = 1e4                                             # huge elements
    lw, lb = 1 + 0.1 * torch.randn((C,), generator=g), 0.1 * torch.randn((C,), generator=g)
    sh, sc = 0.3 * torch.randn((C,), generator=g), 0.3 * torch.randn((C,), generator=g)
    sc[: C // 4] = -1.0                                           # 1 + scale = 0
    w, b = (lw, lb) if mode in ("affine", "both") else (None, None)
    shift, scale = (sh, sc) if mode in ("adaln", "both") else (None, None)
    mod = torch.full((2 * C + 12,), float("nan"))                 # [4 | shift C | 4 | scale C | 4]: NaN around the one row of each
    mod[4:4 + C], mod[8 + C:8 + 2 * C] = sh, sc
    md = mod.to(cuda)
    xbuf = torch.full((rows + 2, C), float("nan"), device=cuda)
    xbuf[:rows] = x.to(cuda)
    obuf = torch.full((rows + 2 * GUARD, C), SENTINEL16, dtype=torch.int16, device=cuda).view(dt)
    dev = lambda t: None if t is None else t.to(cuda)
    kw = dict(ln_w=dev(w), ln_b=dev(b), shift=None if shift is None else md[4:4 + C], scale=None if scale is None else md[8 + C:8 + 2 * C],
              act=act, eps=1e-6, out=obuf[GUARD:GUARD + rows])
    spconv.ln_act(xbuf[:rows], **kw)
    torch.cuda.synchronize()
    first = obuf.clone()
    guard = torch.cat([first[:GUARD], first[GUARD + rows:]]).view(torch.int16)
    assert bool((guard == SENTINEL16).all()), "a store outside the rows of the call"
    spconv.ln_act(xbuf[:rows], **kw)
    assert torch.equal(obuf.view(torch.int16), first.view(torch.int16)), "a second launch gave other bits"
    ref, bnd = S.ln_act_model(x, dt, 1e-6, w, b, shift, scale, act)
    assert torch.isfinite(ref).all() and torch.isfinite(bnd).all()
    n_bad, worst = S.excess(obuf[GUARD:GUARD + rows].cpu(), ref, bnd)
    print(f"ln_act C{C} rows{rows} {mode} act{act} {dt}: worst |err| / bound {worst:.3f}")
    assert n_bad == 0, f"{n_bad} of {rows * C} elements outside the bound (worst {worst:.3g} x)"
