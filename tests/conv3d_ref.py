"""fp64 reference and per-element error bound of the dense 3x3x3 convolution (csrc/conv3d.hip; include/gvf_conv3d.h), of its pixel-shuffle
store and of the occupancy read-out, with the operands the tests share.

A dense volume is a row matrix [B*X*Y*Z, C], row = ((b*X + x)*Y + y)*Z + z.  taps() is the definition: tap k = kx * 9 + ky * 3 + kz of
voxel (b, x, y, z) is the row of (b, x + kx - 1, y + ky - 1, z + kz - 1), a zero row where that is outside the grid.  model() computes in
float64, from the same 16-bit operands, what the kernel computes -- every product of two 16-bit values is exact in float64 -- and bounds
the kernel's own arithmetic in the manner of tests/spconv_ref.py:

  * accumulation: the kernel walks ceil(Cin / 32) chunks of 27 taps, one MFMA k-step each (a zero halo cell adds exact zeros), each step
    counted as one fp32 rounding of a partial sum of magnitude at most S = sum |w x|, one more rounding for the bias and one of slack for
    the MFMA's internal order:  e = (27 ceil(Cin / 32) + 2) 2^-24 (S + |bias|);
  * the addend is one more fp32 add (counted twice, as spconv_ref counts it): 2 2^-24 (|addend| + |acc|);
  * a 16-bit store is bounded by the monotone-rounding interval (gemm_ref._round_bound): a truncating store falls outside it.

Everything is derived; nothing here was measured.  All tensors are torch CPU tensors."""
import math

import torch

from gemm_ref import r16, _round_bound, U32, excess  # noqa: F401

NTAP = 27


def roundup32(c):
    return (c + 31) // 32 * 32


# ---- layout --------------------------------------------------------------------------------------------------------------------------------

def to_rows(dense):
    """[B, C, X, Y, Z] -> [B*X*Y*Z, C]."""
    return dense.permute(0, 2, 3, 4, 1).reshape(-1, dense.shape[1]).contiguous()


def to_dense(rows, grid):
    """[B*X*Y*Z, C] -> [B, C, X, Y, Z]."""
    B, X, Y, Z = grid
    return rows.reshape(B, X, Y, Z, rows.shape[1]).permute(0, 4, 1, 2, 3).contiguous()


# ---- the definition ----------------------------------------------------------------------------------------------------------------------

def taps(x, grid, mutant=None):
    """float64 [27, rows, C]: the operand rows by tap, zeros outside the grid.  The MUTANTS the bound must reject: "periodic" wraps every axis
    (the opposite face in place of the zero padding); "rowshift" takes the neighbour as the row at the flat offset ((kx - 1) Y + ky - 1) Z +
    kz - 1 wherever that row exists (it crosses z, y and sample boundaries)."""
    B, X, Y, Z = grid
    C = x.shape[1]
    v = x.double().reshape(B, X, Y, Z, C)
    out = torch.zeros((NTAP, B * X * Y * Z, C), dtype=torch.float64)
    if mutant == "rowshift":
        flat = x.double()
        n = flat.shape[0]
        for k in range(NTAP):
            off = ((k // 9 - 1) * Y + (k // 3) % 3 - 1) * Z + k % 3 - 1
            lo, hi = max(0, -off), min(n, n - off)
            out[k, lo:hi] = flat[lo + off:hi + off]
        return out
    if mutant == "periodic":
        for k in range(NTAP):
            out[k] = torch.roll(v, shifts=(1 - k // 9, 1 - (k // 3) % 3, 1 - k % 3), dims=(1, 2, 3)).reshape(-1, C)
        return out
    assert mutant is None
    p = torch.zeros((B, X + 2, Y + 2, Z + 2, C), dtype=torch.float64)
    p[:, 1:-1, 1:-1, 1:-1] = v
    for k in range(NTAP):
        kx, ky, kz = k // 9, (k // 3) % 3, k % 3
        out[k] = p[:, kx:kx + X, ky:ky + Y, kz:kz + Z].reshape(-1, C)
    return out


def pixel_shuffle2(rows, grid, reversed_ijk=False):
    """[B*X*Y*Z, C] -> [B*2X*2Y*2Z, C / 8]: channel ((c' 2 + i) 2 + j) 2 + k of voxel (x, y, z) goes to channel c' of voxel (2x + i, 2y + j,
    2z + k).  reversed_ijk: the mutant that reads the three bits as (k, j, i)."""
    B, X, Y, Z = grid
    C = rows.shape[1]
    v = rows.reshape(B, X, Y, Z, C // 8, 2, 2, 2)                   # b x y z c' i j k
    order = (0, 1, 7, 2, 6, 3, 5, 4) if reversed_ijk else (0, 1, 5, 2, 6, 3, 7, 4)
    return v.permute(*order).reshape(B * 8 * X * Y * Z, C // 8).contiguous()


def occupancy(logits, grid, mutant=False):
    """int32 [n, 4] = (b, x, y, z) of the cells with logit > 0 in ascending row order, from a plain loop over the rows.  +0, -0 and NaN are
    not occupied.  mutant: `>= 0`."""
    B, X, Y, Z = grid
    out = []
    for r, v in enumerate(logits.reshape(-1).tolist()):
        if (v >= 0.0) if mutant else (v > 0.0):
            out.append((r // (X * Y * Z), (r // (Y * Z)) % X, (r // Z) % Y, r % Z))
    return torch.tensor(out, dtype=torch.int32).reshape(-1, 4)


def model(x16, grid, w16, bias=None, addend=None, out_dt=None, store="rows", mutant=None, flip=False):
    """(reference, bound), float64 in the output's shape.  x16 16-bit [rows, >= Cin]; w16 16-bit [Cout, Cin, 3, 3, 3]; bias fp32 [Cout];
    addend fp32 in the output's shape; out_dt: None for an fp32 store, else the 16-bit output type; store "rows" or "shuffle2".  flip: the
    mutant with flipped taps (a true convolution)."""
    cout, cin = w16.shape[0], w16.shape[1]
    g = taps(x16[:, :cin], grid, mutant)
    w = w16.double().reshape(cout, cin, NTAP)
    if flip:
        w = w.flip(2)
    acc = torch.zeros((g.shape[1], cout), dtype=torch.float64)
    S = torch.zeros_like(acc)
    for k in range(NTAP):
        acc += g[k] @ w[:, :, k].T
        S += g[k].abs() @ w[:, :, k].abs().T
    b = torch.zeros(cout, dtype=torch.float64) if bias is None else bias.double()
    pre = acc + b
    e = (NTAP * ((cin + 31) // 32) + 2) * U32 * (S + b.abs())
    if store == "shuffle2":
        pre, e = pixel_shuffle2(pre, grid), pixel_shuffle2(e, grid)
    else:
        assert store == "rows"
    if addend is not None:
        a = addend.double()
        e = e + 2.0 * U32 * (a.abs() + pre.abs())
        pre = pre + a
    return pre, _round_bound(pre, e, out_dt)


def reference(*args, **kw):
    return model(*args, **kw)[0]


def bound(*args, **kw):
    return model(*args, **kw)[1]


def flops(grid, cin, cout):
    B, X, Y, Z = grid
    return 2.0 * NTAP * B * X * Y * Z * cin * cout


# ---- operands ------------------------------------------------------------------------------------------------------------------------------

def make_operands(grid, cin, cout, dt, seed, pad=0, store="rows"):
    """x16 [rows, roundup32(cin) + pad] (columns cin .. roundup32(cin) zero -- the kernel reads them --, the `pad` columns after them NaN),
    w16 [cout, cin, 3, 3, 3], the fp32 weight it was rounded from, bias fp32 [cout], addend fp32 in the output's shape -- CPU tensors."""
    B, X, Y, Z = grid
    rows = B * X * Y * Z
    g = torch.Generator().manual_seed(seed)
    x = torch.full((rows, roundup32(cin) + pad), float("nan"))
    x[:, :roundup32(cin)] = 0.0
    x[:, :cin] = torch.randn((rows, cin), generator=g)
    w = torch.randn((cout, cin, 3, 3, 3), generator=g) * (1.0 / math.sqrt(13.5 * cin))
    bias = torch.randn((cout,), generator=g) * 0.5
    shape = (rows * 8, cout // 8) if store == "shuffle2" else (rows, cout)
    addend = torch.randn(shape, generator=g)
    return x.to(dt), w.to(dt), w, bias, addend


def make_logits(grid, seed):
    """fp32 [B, X*Y*Z]: normal values with +0, -0, NaN, +-inf and the smallest subnormals planted at seeded places."""
    B, X, Y, Z = grid
    g = torch.Generator().manual_seed(seed)
    v = torch.randn((B * X * Y * Z,), generator=g)
    special = [0.0, -0.0, float("nan"), float("inf"), float("-inf"), 2.0 ** -149, -2.0 ** -149]
    at = torch.randperm(v.numel(), generator=g)
    n = min(v.numel() // 2, 10 * len(special))
    for i in range(n):
        v[at[i]] = special[i % len(special)]
    return v.reshape(B, X * Y * Z)
