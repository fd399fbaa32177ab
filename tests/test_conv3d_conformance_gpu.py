"""Element-wise conformance of the dense 3x3x3 convolution family (csrc/conv3d.hip; include/gvf_conv3d.h) against the host reference and
bound of tests/conv3d_ref.py (which tests/test_conv3d_ref.py checks on the CPU): every output of the convolution within bound() for both
operand types, both stores and the pixel-shuffle store, on grids smaller than a brick, with partial bricks on every axis, with two samples
and large enough for every tile shape the dispatcher has; NaN containment; buffer edges; equal bits; the occupancy read-out exactly."""
import pytest
import torch

import conv3d_ref as C
from gvfdiffusion_amd.ops import conv3d

pytestmark = pytest.mark.gpu
DTYPES = [torch.bfloat16, torch.float16]
SENTINEL16 = 0x7E5A
GUARD = 8                                   # rows around both buffers: 8 rows of any width keep the views 16-byte aligned

G1, G3, G4, G567, G8, G16 = (1, 1, 1, 1), (1, 3, 3, 3), (1, 4, 4, 4), (1, 5, 6, 7), (2, 8, 8, 8), (1, 16, 16, 16)
GBIG = (2, 24, 16, 24)                      # 288 bricks: the launch keeps two and four channel fragments per wave (Cout 128, 256)

_models = {}


def _model(grid, cin, cout, dt, with_bias, with_addend, store, pad):
    """Operands and the float64 (pre-store value, pre-store bound): computed once per case and operand type, shared, never modified."""
    key = (grid, cin, cout, dt, with_bias, with_addend, store, pad)
    if key not in _models:
        x16, w16, w32, bias, addend = C.make_operands(grid, cin, cout, dt, seed=cin + 3 * cout + grid[1], pad=pad, store=store)
        bias = bias if with_bias else None
        addend = addend if with_addend else None
        pre, e = C.model(x16, grid, w16, bias, addend, None, store)
        _models[key] = (x16, w32, bias, addend, pre, e)
    return _models[key]


def _run(cuda, grid, cin, cout, dt, out_dt, with_bias, with_addend, store="rows", pad=8):
    """-> (device output buffer with guards, reference, bound, call arguments).  Both buffers are views into larger allocations: NaN rows
    around the operand (and NaN columns beyond roundup32(cin)), a sentinel around the output."""
    x16, w32, bias, addend, pre, e = _model(grid, cin, cout, dt, with_bias, with_addend, store, pad)
    bnd = C._round_bound(pre, e, None if out_dt is torch.float32 else dt)
    rows = x16.shape[0]
    orows, ocols = pre.shape
    xbuf = torch.full((rows + 2 * GUARD, x16.shape[1]), float("nan"), dtype=dt, device=cuda)
    xbuf[GUARD:GUARD + rows] = x16.to(cuda)
    wimg = conv3d.pack_weight(w32.to(cuda), dt)
    dev = lambda t: None if t is None else t.to(cuda)
    if out_dt is torch.float32:
        obuf = torch.full((orows + 2 * GUARD, ocols), float("nan"), dtype=torch.float32, device=cuda)
    else:
        obuf = torch.full((orows + 2 * GUARD, ocols), SENTINEL16, dtype=torch.int16, device=cuda).view(dt)
    args = (xbuf[GUARD:GUARD + rows], grid, wimg, cin, cout)
    kw = dict(bias=dev(bias), addend=dev(addend), out_dtype=out_dt, store=store, out=obuf[GUARD:GUARD + orows])
    conv3d.conv3(*args, **kw)
    torch.cuda.synchronize()
    return obuf, pre, bnd, args, kw


def _check(obuf, ref, bnd, what):
    n = ref.shape[0]
    out = obuf[GUARD:GUARD + n].cpu()
    guard = torch.cat([obuf[:GUARD], obuf[GUARD + n:]]).cpu()
    if obuf.dtype is torch.float32:
        assert bool(torch.isnan(guard).all()), "a store outside the rows of the call"
    else:
        assert bool((guard.view(torch.int16) == SENTINEL16).all()), "a store outside the rows of the call"
    assert torch.isfinite(out.float()).all(), f"{what}: a padding column, a row outside the volume or an unwritten element"
    n_bad, worst = C.excess(out, ref, bnd)
    print(f"conv3d {what}: worst |err| / bound {worst:.3f}")
    assert n_bad == 0, f"{what}: {n_bad} of {out.numel()} elements outside the bound (worst {worst:.3g} x)"


CASES = [
    # grid, cin, cout, bias, addend
    (G1, 8, 1, True, False), (G1, 64, 64, False, True), (G1, 160, 80, True, True),
    (G3, 32, 16, True, True), (G3, 8, 48, False, False), (G3, 64, 128, True, False),
    (G4, 64, 80, True, False), (G4, 160, 128, False, True), (G4, 8, 1, False, True), (G4, 32, 32, True, True),
    (G567, 8, 64, True, True), (G567, 32, 1, True, False), (G567, 160, 48, False, True), (G567, 64, 16, True, False), (G567, 32, 32, False, False),
    (G8, 8, 128, True, False), (G8, 32, 80, False, True), (G8, 64, 1, True, True), (G8, 160, 16, True, True), (G8, 64, 48, True, False),
    (G16, 32, 32, True, True), (G16, 8, 64, True, False), (G16, 160, 1, False, False), (G16, 64, 128, True, True),
    (GBIG, 8, 128, True, False), (GBIG, 8, 256, True, True),
]


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("out32", [True, False], ids=["f32out", "lpout"])
@pytest.mark.parametrize("grid,cin,cout,with_bias,with_addend", CASES)
def test_conv_every_element_within_bound(cuda, dt, out32, grid, cin, cout, with_bias, with_addend):
    out_dt = torch.float32 if out32 else dt
    obuf, ref, bnd, _, _ = _run(cuda, grid, cin, cout, dt, out_dt, with_bias, with_addend)
    _check(obuf, ref, bnd, f"{cin}->{cout} grid{grid} bias{int(with_bias)} add{int(with_addend)} {dt} -> {out_dt}")


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("out32", [True, False], ids=["f32out", "lpout"])
@pytest.mark.parametrize("grid,cin,cout,with_bias,with_addend", [
    (G567, 32, 64, True, False), (G8, 8, 8, True, True), (G3, 64, 64, False, True), (G1, 8, 8, False, False), (G16, 64, 64, True, False),
    (GBIG, 8, 256, True, False)])
def test_shuffle2_store_every_element_within_bound(cuda, dt, out32, grid, cin, cout, with_bias, with_addend):
    out_dt = torch.float32 if out32 else dt
    obuf, ref, bnd, _, _ = _run(cuda, grid, cin, cout, dt, out_dt, with_bias, with_addend, store="shuffle2")
    assert ref.shape == (8 * grid[0] * grid[1] * grid[2] * grid[3], cout // 8)
    _check(obuf, ref, bnd, f"shuffle2 {cin}->{cout} grid{grid} bias{int(with_bias)} add{int(with_addend)} {dt} -> {out_dt}")


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("cin,cout", [(64, 128), (8, 32), (32, 1)])
def test_nan_voxel_poisons_exactly_its_neighbours(cuda, dt, cin, cout):
    """One NaN voxel on a brick boundary in sample 0 and one in a corner of sample 1: exactly their 27 and 8 neighbours' outputs are NaN."""
    grid = G8
    B, X, Y, Z = grid
    x16, w16, w32, bias, _ = C.make_operands(grid, cin, cout, dt, seed=21)
    row = lambda b, x, y, z: ((b * X + x) * Y + y) * Z + z
    bad = [(0, 3, 4, 4), (1, 0, 0, 7)]
    for v in bad:
        x16[row(*v), :cin] = float("nan")
    out = conv3d.conv3(x16.to(cuda), grid, conv3d.pack_weight(w32.to(cuda), dt), cin, cout, bias=bias.to(cuda)).cpu()
    near = torch.zeros((B, X, Y, Z), dtype=torch.bool)
    for b, x, y, z in bad:
        near[b, max(x - 1, 0):x + 2, max(y - 1, 0):y + 2, max(z - 1, 0):z + 2] = True
    near = near.reshape(-1)
    assert int(near.sum()) == 27 + 8
    assert bool(torch.isnan(out[near]).all()), "a neighbour of the NaN voxel has finite outputs"
    assert bool(torch.isfinite(out[~near]).all()), "the NaN voxel reached a voxel that is not its neighbour"
    for v in bad:
        x16[row(*v)] = 0
    ref, bnd = C.model(x16, grid, w16, bias)
    assert C.excess(out[~near], ref[~near], bnd[~near])[0] == 0


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("cin,cout,store", [(64, 128, "rows"), (32, 32, "rows"), (32, 64, "shuffle2")])
def test_equal_bits_twice_and_on_two_streams(cuda, dt, cin, cout, store):
    obuf, ref, _, args, kw = _run(cuda, G567, cin, cout, dt, torch.float32, True, True, store=store)
    first = obuf.clone()
    conv3d.conv3(*args, **kw)
    torch.cuda.synchronize()
    assert torch.equal(obuf.view(torch.int32), first.view(torch.int32)), "a second launch gave other bits"
    outs = [torch.empty_like(kw["out"]) for _ in range(2)]
    streams = [torch.cuda.Stream(device=cuda) for _ in range(2)]
    torch.cuda.synchronize()
    for _ in range(3):
        for s, o in zip(streams, outs):
            with torch.cuda.stream(s):
                conv3d.conv3(*args, **dict(kw, out=o))
    torch.cuda.synchronize()
    want = first[GUARD:GUARD + ref.shape[0]].view(torch.int32)
    assert all(torch.equal(o.view(torch.int32), want) for o in outs), "two streams gave other bits"


@pytest.mark.parametrize("grid,kind", [
    (G567, "mixed"), (G1, "mixed"), ((2, 13, 11, 9), "mixed"), (G16, "mixed"), ((2, 16, 16, 16), "mixed"),
    ((2, 13, 11, 9), "none"), ((2, 13, 11, 9), "all"), (G1, "none"), (G1, "all"), ((1, 2, 1024, 1), "mixed")])
def test_occupancy_coords_equal_argwhere(cuda, grid, kind):
    """(2, 13, 11, 9): 2574 cells, one workgroup span of 2048 and a partial one; +-0, NaN, +-inf and subnormals among the mixed logits."""
    B, X, Y, Z = grid
    logits = C.make_logits(grid, seed=X + Y)
    if kind == "none":
        logits = -logits.abs()                              # -0, NaN and negative values
    elif kind == "all":
        logits = torch.nan_to_num(logits.abs(), nan=1.0) + 2.0 ** -149
    dense = logits.reshape(B, 1, X, Y, Z)
    want = torch.argwhere(dense > 0)[:, [0, 2, 3, 4]].int()
    got = conv3d.occupancy_coords(logits.to(cuda), grid)
    again = conv3d.occupancy_coords(logits.to(cuda), grid)
    assert got.dtype == torch.int32 and got.dim() == 2 and got.shape[1] == 4
    assert torch.equal(got.cpu(), want), f"{got.shape[0]} rows, want {want.shape[0]}"
    assert torch.equal(got, again)
    if kind == "none":
        assert got.shape[0] == 0
    if kind == "all":
        assert got.shape[0] == B * X * Y * Z
