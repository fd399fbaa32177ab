"""Element-wise conformance of the unfused link the row-block launch is compared with elsewhere: gvf_layernorm_modulate (csrc/elem.hip:
ln_mod_kernel for C = 256, 512, 768, 1024, ln_mod_generic_kernel for every other C) against the LayerNorm band of tests/rowblock_ref.py with
that kernel's rounding counts, and gvf_cast_pad against the correctly rounded cast / SiLU.  Rows that are no multiple of the four rows of a
workgroup, rows_per_group that does not divide the rows, affine / adaLN / both, adversarial rows (a common offset of 100 standard deviations,
constant rows, one huge element, scale = -1), guard rows around the output, NaN in every padding the contract allows, the same bits on a
second launch."""
import pytest
import torch

import rowblock_ref as R
from gvfdiffusion_amd import _lib
from gvfdiffusion_amd.ops import dit_ops

pytestmark = pytest.mark.gpu
SENTINEL16 = 0x7E5A
DTYPES = [torch.bfloat16, torch.float16]
GUARD = 5


def _rows(C, rows, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((rows, C), generator=g) * 2 + 0.5
    x[0:3] += 200.0                                               # |mean| = 100 x std
    for r, v in zip(range(3, min(6, rows)), (3.0, -0.37, 0.0)):
        x[r] = v                                                  # variance 0: eps decides
    x[6:8, 1::29] = 1e4                                           # huge elements
    return g, x


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("mode", ["affine", "adaln", "both"])
@pytest.mark.parametrize("C,rows,rpg", [(256, 37, 10), (512, 1, 1), (768, 53, 53), (1024, 130, 48), (64, 37, 10), (100, 6, 4), (1028, 41, 7)])
def test_layernorm_modulate_elementwise(cuda, dt, mode, C, rows, rpg):
    g, x = _rows(C, rows, C + rows)
    groups = (rows + rpg - 1) // rpg
    ld = 2 * C + 12                                               # [4 | shift C | 4 | scale C | 4]
    mod = torch.full((groups, ld), float("nan"))
    mod[:, 4:4 + C] = torch.randn((groups, C), generator=g) * 0.3
    mod[:, 8 + C:8 + 2 * C] = torch.randn((groups, C), generator=g) * 0.3
    mod[-1, 8 + C:8 + C + C // 2] = -1.0                          # mul = 0 in half of the last group's columns
    lw, lb = 1 + 0.1 * torch.randn((C,), generator=g), 0.1 * torch.randn((C,), generator=g)
    shift, scale = (mod[:, 4:], mod[:, 8 + C:]) if mode != "affine" else (None, None)
    w, b = (lw, lb) if mode != "adaln" else (None, None)
    xbuf = torch.full((rows + 3, C), float("nan"), device=cuda)
    xbuf[:rows] = x.to(cuda)
    md = mod.to(cuda)
    obuf = torch.full((rows + 2 * GUARD, C), SENTINEL16, dtype=torch.int16, device=cuda).view(dt)
    out = obuf[GUARD:GUARD + rows]
    dev = lambda t: None if t is None else t.to(cuda)
    args = (1e-6, dev(w), dev(b), None if shift is None else md[:, 4:], None if scale is None else md[:, 8 + C:], ld, rpg)
    dit_ops.layernorm_modulate(xbuf[:rows], out, *args)
    torch.cuda.synchronize()
    first = obuf.clone()
    guard = torch.cat([first[:GUARD], first[GUARD + rows:]]).view(torch.int16)
    assert bool((guard == SENTINEL16).all()), "a store outside the rows of the call"
    dit_ops.layernorm_modulate(xbuf[:rows], out, *args)
    assert torch.equal(obuf.view(torch.int16), first.view(torch.int16)), "a second launch gave other bits"
    a16, amb, bnd = R.ln_band(x, dt, 1e-6, w, b, shift, scale, rpg, kernel="elem")
    assert torch.isfinite(a16.float()).all() and torch.isfinite(bnd).all()
    n_bad, worst = R.excess(out.cpu(), a16.double(), bnd)
    print(f"layernorm_modulate C{C} rows{rows} {mode} {dt}: worst |err| / bound {worst:.3f}, ambiguous outputs {100 * R.ambiguous_share(amb):.3f} %")
    assert n_bad == 0, f"{n_bad} of {rows * C} elements outside the bound (worst {worst:.3g} x)"


def test_layernorm_modulate_refuses_misaligned_vectors_on_the_float4_path(cuda):
    """ln_w / ln_b / shift / scale that are not 16-byte aligned are refused where the float4 kernel would load them (C % 256 == 0, C <= 1024)
    -- nothing is launched -- and accepted where the generic kernel reads them one value at a time."""
    rows, dt = 8, torch.bfloat16
    for C, fast in ((512, True), (1024, True), (100, False)):
        x = torch.randn((rows, C)).to(cuda)
        out = torch.full((rows, C), SENTINEL16, dtype=torch.int16, device=cuda).view(dt)
        vec = torch.randn((2 * C + 8,)).to(cuda)
        table = torch.randn((1, 2 * C + 8)).to(cuda)
        bad = [dict(ln_w=vec[1:], ln_b=vec[C + 4:]), dict(ln_w=vec[0:], ln_b=vec[C + 2:]), dict(shift=table[:, 1:], scale=table[:, C + 4:], mod_ld=2 * C + 8, rows_per_group=rows),
               dict(shift=table[:, 0:], scale=table[:, C + 3:], mod_ld=2 * C + 8, rows_per_group=rows)]
        for kw in bad:
            if fast:
                with pytest.raises(_lib.GvfError):
                    dit_ops.layernorm_modulate(x, out, 1e-6, **kw)
                torch.cuda.synchronize()
                assert bool((out.view(torch.int16) == SENTINEL16).all())
            else:
                dit_ops.layernorm_modulate(x, out, 1e-6, **kw)
                torch.cuda.synchronize()
                assert torch.isfinite(out.float()).all()
        dit_ops.layernorm_modulate(x, out, 1e-6, ln_w=vec[0:], ln_b=vec[C + 4:])       # aligned: accepted
        torch.cuda.synchronize()
        assert torch.isfinite(out.float()).all()


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("rows,cols,ld_src,ld_dst", [(5, 14, 14, 64), (37, 21, 23, 24), (100003, 21, 23, 24), (3, 512, 520, 512)])
def test_cast_pad_elementwise(cuda, dt, act, rows, cols, ld_src, ld_dst):
    """The cast is exact (the correctly rounded 16-bit value, bit for bit); SiLU within the bound of its fp32 arithmetic, with the right signed
    zero / v where __expf(-v) overflows or vanishes; padding columns exactly zero; NaN in the source's padding never read; 100003 rows of 24
    make the grid-stride loop wrap."""
    g = torch.Generator().manual_seed(rows + cols + act)
    v = torch.randn((rows, cols), generator=g) * 3
    v[0, :6] = torch.tensor([-200.0, -95.0, -88.0, 90.0, 200.0, 0.0])
    v[-1, :4] = torch.tensor([-20.0, 20.0, 1e-5, -1e-5])
    src = torch.full((rows, ld_src), float("nan"), device=cuda)
    src[:, :cols] = v.to(cuda)
    obuf = torch.full((rows + 2 * GUARD, ld_dst), SENTINEL16, dtype=torch.int16, device=cuda).view(dt)
    out = obuf[GUARD:GUARD + rows]
    dit_ops.cast_pad(src[:, :cols], ld_dst, act=act, out=out)
    torch.cuda.synchronize()
    first = obuf.clone()
    guard = torch.cat([first[:GUARD], first[GUARD + rows:]]).view(torch.int16)
    assert bool((guard == SENTINEL16).all()), "a store outside the rows of the call"
    dit_ops.cast_pad(src[:, :cols], ld_dst, act=act, out=out)
    assert torch.equal(obuf.view(torch.int16), first.view(torch.int16)), "a second launch gave other bits"
    o = out.cpu()
    assert bool((o[:, cols:].view(torch.int16) == 0).all()), "padding columns are not +0"
    ref, bnd = R.cast_model(v, dt, act)
    n_bad, worst = R.excess(o[:, :cols], ref, bnd)
    print(f"cast_pad act{act} {rows}x{cols} {dt}: worst |err| / bound {worst:.3f}")
    assert n_bad == 0, f"{n_bad} elements outside the bound (worst {worst:.3g} x)"
    if act == 0:
        assert torch.equal(o[:, :cols].view(torch.int16), v.to(dt).view(torch.int16)), "the cast is not the correctly rounded value"
    else:
        bits = o[0, :6].view(torch.int16).tolist()
        assert bits[0] == bits[1] == -32768, "v / (1 + inf) must be -0"
        assert bits[3:5] == torch.tensor([90.0, 200.0]).to(dt).view(torch.int16).tolist() and bits[5] == 0
