"""fp64 reference and per-element error bound of the submanifold sparse 3x3x3 convolution (csrc/spconv.hip; include/gvf_spconv.h) and of
its LayerNorm + activation link, with the voxel sets the tests share.

neighbor_map() is the definition, from a Python dict: row j is tap k = kx * 9 + ky * 3 + kz of row i when its coordinates are
(b, x + kx - 1, y + ky - 1, z + kz - 1).  reference() computes in float64, from the same 16-bit operands, what the kernel computes: every
product of two 16-bit values is exact in float64.  bound() follows the kernel's arithmetic in the manner of tests/gemm_ref.py:

  * accumulation: the kernel walks 27 taps of ceil(Cin / 32) MFMA k-steps (a skipped tap adds nothing, a zero row adds exact zeros), each
    step counted as one fp32 rounding of a partial sum of magnitude at most S = sum |w x| over the PRESENT neighbours, one more rounding
    for the bias and one of slack for the MFMA's internal order:  e = (27 ceil(Cin / 32) + 2) 2^-24 (S + |bias|);
  * the addend is one more fp32 add (counted twice, as gemm_ref counts the residual update): 2 2^-24 (|addend| + |acc|);
  * a 16-bit store is bounded by the monotone-rounding interval (gemm_ref._round_bound): a truncating store falls outside it.

Everything is derived; nothing here was measured.  All tensors are torch CPU tensors."""
import math

import numpy as np
import torch

from gemm_ref import r16, _round_bound, U32, excess  # noqa: F401
import rowblock_ref as R

NTAP = 27
SILU_LIP = 1.1                       # max |d/dx silu(x)| = 1.0998 at x = 2.4


# ---- voxel sets ------------------------------------------------------------------------------------------------------------------------

def shell(res, r_in, r_out, batch=0):
    """int32 [n,4] (batch, x, y, z): the cells of a res^3 grid whose centre lies r_in <= |p - c| < r_out from the grid's centre, grid order."""
    g = torch.arange(res, dtype=torch.float64) + 0.5 - res / 2.0
    x, y, z = torch.meshgrid(g, g, g, indexing="ij")
    d = torch.sqrt(x * x + y * y + z * z)
    idx = torch.nonzero((d >= r_in) & (d < r_out)).int()
    return torch.cat([torch.full((idx.shape[0], 1), batch, dtype=torch.int32), idx], dim=1).contiguous()


def standard_coords(permuted=False, seed=7):
    """shell(16, 4.5, 6.0) in sample 0 and shell(16, 2.0, 5.5) in sample 1: 552 + 640 = 1192 rows; permuted: a seeded random order of
    each sample's rows (samples stay contiguous)."""
    parts = [shell(16, 4.5, 6.0, 0), shell(16, 2.0, 5.5, 1)]
    if permuted:
        g = torch.Generator().manual_seed(seed)
        parts = [p[torch.randperm(p.shape[0], generator=g)] for p in parts]
    return torch.cat(parts).contiguous()


def block_coords(n, batch=0, origin=(0, 0, 0)):
    g = torch.arange(n, dtype=torch.int32)
    x, y, z = torch.meshgrid(g + origin[0], g + origin[1], g + origin[2], indexing="ij")
    c = torch.stack([x, y, z], dim=-1).reshape(-1, 3)
    return torch.cat([torch.full((c.shape[0], 1), batch, dtype=torch.int32), c], dim=1).contiguous()


def edge_sets():
    """name -> int32 [T,4]: the sets of the conformance family beside the standard input."""
    sets = {"one": torch.tensor([[0, 5, 6, 7]], dtype=torch.int32)}
    solid = block_coords(4)                                                          # 64 cells
    sets["t63"], sets["t64"] = solid[:63].contiguous(), solid
    sets["t65"] = torch.cat([solid, torch.tensor([[0, 4, 0, 0]], dtype=torch.int32)])
    sets["solid6"] = block_coords(6, origin=(3, 1, 2))
    c8 = block_coords(8)
    sets["checker"] = (c8 * torch.tensor([1, 2, 2, 2], dtype=torch.int32)).contiguous()      # stride 2: only the centre tap exists
    # cells at 0 and 1023 on every axis, and decoys exactly where a wrapped 10-bit key would land: (x - 1) & 1023 = 1023 for x = 0 and
    # (x + 1) & 1023 = 0 for x = 1023 put the opposite face next door; a carry out of z into y (z + 1 = 1024 -> y + 1, z = 0) and a
    # borrow (z - 1 = -1 -> y - 1, z = 1023) are there too
    cells = []
    for a in (0, 1023):
        for b in (0, 1023):
            for c in (0, 1023):
                cells.append((0, a, b, c))
    cells += [(0, 5, 5, 1023), (0, 5, 6, 0), (0, 5, 4, 1023), (0, 5, 5, 0), (0, 6, 0, 0), (0, 5, 1023, 1023),
              (0, 1023, 500, 1023), (0, 0, 501, 0), (0, 0, 500, 0), (0, 1023, 499, 1023), (0, 1022, 1023, 1023), (0, 1, 0, 0)]
    sets["faces"] = torch.tensor(sorted(set(cells)), dtype=torch.int32)
    twin = shell(8, 1.0, 3.5, 0)
    twin1 = twin.clone()
    twin1[:, 0] = 1
    sets["twins"] = torch.cat([twin, twin1]).contiguous()                            # two samples, identical (x, y, z)
    return sets


# ---- the definition ----------------------------------------------------------------------------------------------------------------------

def neighbor_map(coords, wrap10=False, cross_sample=False):
    """int32 [T,27] from a dict.  The two switches build the MUTANTS the bound must reject: wrap10 packs the neighbour's coordinates
    into 10 bits each without a range test (-1 -> 1023, 1024 -> 0); cross_sample ignores the batch index."""
    c = coords.tolist()
    if wrap10:
        key = lambda b, x, y, z: (b << 30) | ((x & 1023) << 20) | ((y & 1023) << 10) | (z & 1023)      # an unguarded packing
    elif cross_sample:
        key = lambda b, x, y, z: (x, y, z)
    else:
        key = lambda b, x, y, z: (b, x, y, z)
    table = {}
    for i, (b, x, y, z) in enumerate(c):
        table[key(b, x, y, z)] = i
    out = np.full((len(c), NTAP), -1, dtype=np.int32)
    for i, (b, x, y, z) in enumerate(c):
        for k in range(NTAP):
            nx, ny, nz = x + k // 9 - 1, y + (k // 3) % 3 - 1, z + k % 3 - 1
            if not wrap10 and not (0 <= nx < 1024 and 0 <= ny < 1024 and 0 <= nz < 1024):
                continue
            out[i, k] = table.get(key(b, nx, ny, nz), -1)
    return torch.from_numpy(out)


def _gathered(x16, nbr, cin):
    """fp64 [T, 27, cin]: the operand rows by neighbour, zeros where absent."""
    x = x16[:, :cin].double()
    idx = nbr.long().clamp_min(0)
    g = x[idx.reshape(-1)].reshape(nbr.shape[0], NTAP, cin)
    return g * (nbr >= 0).double()[:, :, None]


def model(x16, nbr, w16, bias=None, addend=None, out_dt=None):
    """(reference, bound), float64 [T, Cout].  x16 16-bit [T, >= Cin]; w16 16-bit [Cout,3,3,3,Cin]; bias fp32 [Cout]; addend fp32
    [T, Cout]; out_dt: None for an fp32 store, else the 16-bit output type."""
    cout, cin = w16.shape[0], w16.shape[4]
    g = _gathered(x16, nbr, cin).reshape(nbr.shape[0], NTAP * cin)
    w = w16.double().reshape(cout, NTAP * cin)
    acc = g @ w.T
    S = g.abs() @ w.abs().T
    b = torch.zeros(cout, dtype=torch.float64) if bias is None else bias.double()
    pre = acc + b
    e = (NTAP * ((cin + 31) // 32) + 2) * U32 * (S + b.abs())
    if addend is not None:
        a = addend.double()
        e = e + 2.0 * U32 * (a.abs() + pre.abs())
        pre = pre + a
    return pre, _round_bound(pre, e, out_dt)


def reference(x16, nbr, w16, bias=None, addend=None, out_dt=None):
    return model(x16, nbr, w16, bias, addend, out_dt)[0]


def bound(x16, nbr, w16, bias=None, addend=None, out_dt=None):
    return model(x16, nbr, w16, bias, addend, out_dt)[1]


def dense_conv3d(x16, coords, w16, bias=None):
    """float64 F.conv3d on the densified grid, read back at the active sites: the definition's other form."""
    cin = w16.shape[4]
    c = coords.long()
    B = int(c[:, 0].max()) + 1
    lo = c[:, 1:].min(0).values
    ext = (c[:, 1:].max(0).values - lo + 1).tolist()
    grid = torch.zeros((B, cin, *ext), dtype=torch.float64)
    p = c[:, 1:] - lo
    grid[c[:, 0], :, p[:, 0], p[:, 1], p[:, 2]] = x16[:, :cin].double()
    y = torch.nn.functional.conv3d(grid, w16.double().permute(0, 4, 1, 2, 3), None if bias is None else bias.double(), padding=1)
    return y[c[:, 0], :, p[:, 0], p[:, 1], p[:, 2]]


def flops_present(nbr, cin, cout):
    return 2.0 * float((nbr >= 0).sum()) * cin * cout


# ---- LayerNorm + activation (gvf_ln_act_rows) -----------------------------------------------------------------------------------------------

def ln_act_model(X, dt, eps, ln_w=None, ln_b=None, shift=None, scale=None, act=0):
    """(reference 16-bit value as float64, bound on |stored - reference|).  The LayerNorm part is the bar of tests/test_elem_conformance_gpu.py
    (rowblock_ref.ln_model, kernel="elem": the kernel sums as elem.hip does); SiLU adds what rowblock_ref.cast_model counts for
    v / (1 + __expf(-v)) and carries the LayerNorm's error through |silu'| <= 1.1.  shift, scale: one row of C each."""
    M = X.shape[0]
    sh = None if shift is None else shift.reshape(1, -1)
    sc = None if scale is None else scale.reshape(1, -1)
    a, e_a = R.ln_model(X, eps, ln_w, ln_b, sh, sc, rpg=max(M, 1), kernel="elem")
    if act == 1:
        s = torch.sigmoid(a)
        g = a * s
        e_a = SILU_LIP * e_a + g.abs() * ((1.0 - s) * (2.0 * a.abs() + 4.0) + 3.0) * U32 + 2.0 ** -126 + g.abs() * (a < -88.0)
        a = g
    ref = r16(a, dt)
    hi, lo = r16(a + e_a, dt), r16(a - e_a, dt)
    return ref, torch.maximum(hi - ref, ref - lo)


# ---- operands ------------------------------------------------------------------------------------------------------------------------------

def make_operands(T, cin, cout, dt, seed, ld_in=None):
    """x16 [T, ld_in] (padding columns NaN), w16 [cout,3,3,3,cin], bias fp32, addend fp32 -- CPU tensors."""
    g = torch.Generator().manual_seed(seed)
    ld_in = cin if ld_in is None else ld_in
    x = torch.full((T, ld_in), float("nan"))
    x[:, :cin] = torch.randn((T, cin), generator=g)
    w = torch.randn((cout, 3, 3, 3, cin), generator=g) * (1.0 / math.sqrt(13.5 * cin))
    bias = torch.randn((cout,), generator=g) * 0.5
    addend = torch.randn((T, cout), generator=g)
    return x.to(dt), w.to(dt), w, bias, addend
