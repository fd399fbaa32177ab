"""Conformance of CLIP's image tower on the device (csrc/clip.hip, GVF_EPI_QUICK_GELU_16 of csrc/gemm.hip, model/clip.py and the alignment
seam) against the float64 restatement of tests/clip_ref.py, which tests/test_clip_ref.py holds to transformers' implementation.

Shapes are the smallest that reach every edge: widths 128, 384 and 768, grids 1 x 1 (one patch: a nearly empty 32-patch tile, 2 tokens), 2 x 2,
3 x 3 at B = 5 (45 patch rows: tiles straddle images, a partial last tile) and the released 7 x 7 (50 tokens), fp16 and bf16, both input kinds."""
import math
from types import SimpleNamespace

import pytest
import torch

import clip_ref as C
import gemm_ref as G
import vit_ref as V
from gvfdiffusion_amd import _lib, synthetic
from gvfdiffusion_amd.model.clip import CLIPVisionTransformer, clip_preprocess_u8
from gvfdiffusion_amd.ops import clip as clip_ops, dit_ops

pytestmark = pytest.mark.gpu
DTYPES = [torch.float16, torch.bfloat16]
IDS = ["fp16", "bf16"]
FRONT = [(128, 1, 1), (128, 2, 3), (384, 3, 5), (768, 7, 2)]          # (D, grid, B)
SENTINEL16 = 0x7E5A
SENTINEL32 = 0x7FA5A5A5


def _bits(t):
    return t.view(torch.int16) if t.element_size() == 2 else t.view(torch.int32)


def _check(out_h, ref, bnd, what):
    n_bad, worst = G.excess(out_h, ref, bnd)
    print(f"{what}: rel_l2 {V.rel_l2(out_h, ref):.2e}, max |err| / bound {worst:.3f}")
    assert n_bad == 0, f"{what}: {n_bad} of {ref.numel()} elements outside the bound (worst {worst:.2f} x)"


def _u8(B, grid, seed=0):
    return torch.randint(0, 256, (B, 3, grid * 32, grid * 32), generator=torch.Generator().manual_seed(200 + seed), dtype=torch.uint8)


def _operand(img, kind, dt):
    """(the tensor the kernel is handed, its 16-bit operand image as float64)"""
    if kind == "u8":
        tab = C.operand_table(dt)
        a = torch.stack([tab[c][img[:, c].long()] for c in range(3)], 1)
        return img, a.double()
    pix = C.normalise_u8(img) + 0.01 * torch.randn(img.shape, generator=torch.Generator().manual_seed(1))      # not on the table's grid
    return pix, pix.to(dt).double()


def _front_args(sd, dt, dev):
    return (clip_ops.pack_patch_weight(sd["conv1.weight"].to(dev), dt), sd["class_embedding"].to(dev), sd["positional_embedding"].to(dev),
            clip_ops.operand_table(dt).to(dev))


def _front_checked(cuda, dt, sd, given, a16, what):
    """patch_embed, then ln_pre as its second launch: both element-wise, both twice."""
    D = sd["class_embedding"].shape[0]
    w, cls, pos, lut = _front_args(sd, dt, cuda)
    assert torch.equal(_bits(w.cpu()), _bits(sd["conv1.weight"].reshape(D, -1).to(dt)))
    dimg = given.to(cuda)
    x = clip_ops.patch_embed(dimg, w, cls, pos, lut)
    x2 = clip_ops.patch_embed(dimg, w, cls, pos, lut)
    torch.cuda.synchronize()
    assert torch.equal(_bits(x), _bits(x2)), f"{what}: a second launch gave other bits"
    xh, B = x.cpu(), given.shape[0]
    n = pos.shape[0] - 1
    assert xh.shape == (B, 1 + n, D)
    assert torch.equal(xh[:, 0], (sd["class_embedding"] + sd["positional_embedding"][0]).expand(B, D)), f"{what}: cls row"
    ref, bnd = C.patch_embed_model(a16, sd, dt)
    _check(xh[:, 1:], ref, bnd, what + " accumulator + pos")
    # ln_pre in place, with the partial statistics of the rows as written
    parts = dit_ops.gemm_stats_parts(D)
    assert parts == D // 64
    lw, lb = sd["ln_pre.weight"].to(cuda), sd["ln_pre.bias"].to(cuda)
    st = torch.empty((B * (1 + n), parts, 2), device=cuda)
    y = clip_ops.ln_rows(x.clone(), lw, lb, C.EPS, st)
    st2 = torch.empty_like(st)
    y2 = clip_ops.ln_rows(x.clone(), lw, lb, C.EPS, st2)
    torch.cuda.synchronize()
    assert torch.equal(_bits(y), _bits(y2)) and torch.equal(_bits(st), _bits(st2)), f"{what}: a second ln_pre gave other bits"
    ref, bnd = V.layernorm_model(xh, C.EPS, sd["ln_pre.weight"], sd["ln_pre.bias"], None)
    yh = y.cpu()
    _check(yh, ref, bnd, what + " ln_pre")
    rows = yh.reshape(-1, parts, 64).double()
    b_sum, b_sq = G.stats_bound(rows.float())
    sth = st.cpu().double()
    assert bool(((sth[..., 0] - rows.sum(-1)).abs() <= b_sum).all()), f"{what}: row sums"
    assert bool(((sth[..., 1] - (rows * rows).sum(-1)).abs() <= b_sq).all()), f"{what}: row sums of squares"
    return xh


# ---- patch embedding + ln_pre --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
@pytest.mark.parametrize("kind", ["u8", "f32"])
@pytest.mark.parametrize("D,grid,B", FRONT)
def test_patch_embed_ln_pre_elementwise(cuda, dt, kind, D, grid, B):
    sd = C.random_state_dict(D, 0, grid, 64, seed=D + grid)
    given, a16 = _operand(_u8(B, grid, B), kind, dt)
    _front_checked(cuda, dt, sd, given, a16, f"clip front {dt} {kind} D{D} grid{grid} B{B}")


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
@pytest.mark.parametrize("kind", ["u8", "f32"])
def test_patch_embed_gather_index(cuda, dt, kind):
    """Pixel values encode (c, y, x) -- (5 c + 7 y + 13 x) mod 251, an integer every operand type holds exactly -- and channel d's weight is
    one-hot at k_d = 977 d mod 3072: out[patch][d] must BE the pixel (c, dy, dx)_d of that patch, bit for bit (position rows zero).  A wrong
    gather index (transposed dy / dx, a channel or chunk stride off, a neighbouring patch) reads another pixel."""
    D, grid, B = 128, 3, 5
    S = grid * 32
    c, y, x = torch.meshgrid(torch.arange(3), torch.arange(S), torch.arange(S), indexing="ij")
    code = ((5 * c + 7 * y + 13 * x) % 251)
    img = torch.stack([(code + 17 * b) % 251 for b in range(B)]).to(torch.uint8)
    sd = C.random_state_dict(D, 0, grid, 64, seed=9)
    ks = (977 * torch.arange(D)) % C.PATCH_K
    w = torch.zeros(D, C.PATCH_K)
    w[torch.arange(D), ks] = 1.0
    sd["conv1.weight"] = w.view(D, 3, 32, 32)
    sd["positional_embedding"] = torch.zeros_like(sd["positional_embedding"])
    if kind == "u8":
        given, a16 = _operand(img, "u8", dt)
    else:
        given = img.float()
        a16 = given.to(dt).double()
        assert torch.equal(a16, given.double())
    xh = _front_checked(cuda, dt, sd, given, a16, f"clip front {dt} {kind} coded pixels")
    want = C.patch_rows(a16)[:, ks].view(B, grid * grid, D)
    assert torch.equal(xh[:, 1:].double(), want)


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_front_with_a_high_norm_position_row(cuda, dt):
    """Three rows (the first patch, a middle one, the last) carry 8 x the typical norm plus a large common offset through their position
    entries: a variance taken as E[x^2] - mean^2 would cancel there; ln_pre takes it from the centred values."""
    D, grid, B = 384, 3, 5
    sd = C.random_state_dict(D, 0, grid, 64, seed=21)
    g = torch.Generator().manual_seed(22)
    for i in (0, 4, 8):
        sd["positional_embedding"][1 + i] += 8.0 * torch.randn(D, generator=g) + 40.0
    given, a16 = _operand(_u8(B, grid, 3), "u8", dt)
    _front_checked(cuda, dt, sd, given, a16, f"clip front {dt} high-norm rows")


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_uint8_path_equals_fp32_path_fed_the_table_values(cuda, dt):
    D, grid, B = 128, 2, 3
    sd = C.random_state_dict(D, 0, grid, 64, seed=5)
    img = _u8(B, grid, 4)
    w, cls, pos, lut = _front_args(sd, dt, cuda)
    tab = C.operand_table(dt).float()
    as_f32 = torch.stack([tab[c][img[:, c].long()] for c in range(3)], 1)
    a = clip_ops.patch_embed(img.to(cuda), w, cls, pos, lut)
    b = clip_ops.patch_embed(as_f32.to(cuda), w, cls, pos, None)
    assert torch.equal(_bits(a), _bits(b))


# ---- the QuickGELU epilogue -----------------------------------------------------------------------------------------------------------------
def _filled(shape, dt, dev):
    return torch.full(shape, SENTINEL16, dtype=torch.int16, device=dev).view(dt)


def _launch_checked(obuf, launch, region, what):
    before = obuf.clone()
    launch()
    torch.cuda.synchronize()
    after = obuf.clone()
    mask = torch.ones(obuf.shape, dtype=torch.bool, device=obuf.device)
    mask[:region[0], :region[1]] = False
    assert torch.equal(_bits(after)[mask], _bits(before)[mask]), f"{what}: a store outside [M, N]"
    obuf.copy_(before)
    launch()
    assert torch.equal(_bits(obuf), _bits(after)), f"{what}: a second launch gave other bits"
    return after


def _extremes(out, ref_pre, dt, what):
    """columns 2 / 3 hold pre-activations of +-65504 in the last row: finite, +65504 passes through, -65504 gives -0"""
    assert torch.isfinite(out.float()).all(), f"{what}: a non-finite output"
    assert float(ref_pre[-1, 2]) == 65504.0 and float(ref_pre[-1, 3]) == -65504.0
    assert float(out[-1, 2]) == float(torch.tensor(65504.0).to(dt)), f"{what}: v = +65504"
    neg = out[-1, 3].float()
    assert float(neg) == 0.0 and bool(torch.signbit(neg)), f"{what}: v = -65504 must give -0, got {float(neg)}"


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
@pytest.mark.parametrize("M", [6, 30, 90])
def test_quick_gelu_epilogue_gemm(cuda, dt, M):
    N, K = 512, 128
    g = torch.Generator().manual_seed(M)
    a_h = (3.0 * torch.randn((M, K), generator=g)).to(dt)
    w_h = (torch.randn((N, K), generator=g) / math.sqrt(K)).to(dt)
    bias = torch.randn((N,), generator=g)
    bias[::64] = 40.0                                                      # exp(-68): the sigmoid is 1 to fp32
    bias[1::64] = -70.0                                                    # exp(+100 and more): expf overflows in part of the column
    # the ACCUMULATOR reaches +-65504 in the last row: a = (256, 128, ... 0.25, 0 ...), w = +-128 on those 11 columns: 128 * 511.75, every
    # operand a power of two (exact in fp16 and bf16), every partial sum exact in fp32
    a_h[-1] = 0
    a_h[-1, :11] = 2.0 ** torch.arange(8, -3, -1)
    w_h[2:4] = 0
    w_h[2, :11], w_h[3, :11] = 128.0, -128.0
    bias[2], bias[3] = 0.0, 0.0
    obuf = _filled((M + 2, N + 8), dt, cuda)
    a, w, b = a_h.to(cuda), w_h.to(cuda), bias.to(cuda)
    after = _launch_checked(obuf, lambda: dit_ops.gemm(a, w, b, obuf[:M, :N], dit_ops.EPI_QUICK_GELU_16), (M, N), f"quick_gelu gemm {dt} M{M}")
    ref, bnd = C.quick_gelu_model(a_h, w_h, bias)
    pre = a_h.double() @ w_h.double().T + bias.double()
    assert float(pre[:-1].max()) > 30.0 and float(pre[:-1].min()) < -60.0
    out = after[:M, :N].cpu()
    _extremes(out, pre, dt, f"quick_gelu gemm {dt} M{M}")
    _check(out, ref, bnd, f"quick_gelu gemm {dt} M{M}")


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
@pytest.mark.parametrize("M", [6, 30, 90])
def test_quick_gelu_epilogue_gemm_ln(cuda, dt, M):
    """The same epilogue behind the LayerNorm-folded operand (the MLP's c_fc): statistics from gvf_clip_ln_rows, as in the model's block 0.  The
    +-65504 pre-activations come through the bias (the operand of this path is a normalised row)."""
    N, K = 512, 128
    g = torch.Generator().manual_seed(1000 + M)
    x = (2.0 * torch.randn((M, K), generator=g) + 0.3).to(cuda)
    parts = dit_ops.gemm_stats_parts(K)
    stats = torch.empty((M, parts, 2), device=cuda)
    pre_w, pre_b = (1.0 + 0.1 * torch.randn(K, generator=g)).to(cuda), (0.1 * torch.randn(K, generator=g)).to(cuda)
    clip_ops.ln_rows(x, pre_w, pre_b, C.EPS, stats)
    w_h = (3.0 * torch.randn((N, K), generator=g) / math.sqrt(K)).to(dt)
    bias = torch.randn((N,), generator=g)
    bias[::64] = 40.0
    bias[1::64] = -70.0
    w_h[2:4] = 0
    bias[2], bias[3] = 65504.0, -65504.0
    ln_w, ln_b = 1.0 + 0.2 * torch.randn(K, generator=g), 0.2 * torch.randn(K, generator=g)
    obuf = _filled((M + 2, N + 8), dt, cuda)
    w, b, lw, lb = w_h.to(cuda), bias.to(cuda), ln_w.to(cuda), ln_b.to(cuda)
    after = _launch_checked(obuf, lambda: dit_ops.gemm_ln_bf16(x, stats, parts, w, b, obuf[:M, :N], dit_ops.EPI_QUICK_GELU_16, eps=C.EPS, ln_w=lw,
                                                               ln_b=lb), (M, N), f"quick_gelu gemm_ln {dt} M{M}")
    a16, amb = G.ln_operand(x.cpu(), parts, dt, C.EPS, ln_w, ln_b)
    ref, bnd = C.quick_gelu_model(a16, w_h, bias, a_err=amb.abs() @ w_h.double().abs().T)
    pre = a16.double() @ w_h.double().T + bias.double()
    assert float(pre.max()) > 30.0 and float(pre[:, 4:].min()) < -60.0
    out = after[:M, :N].cpu()
    _extremes(out, pre, dt, f"quick_gelu gemm_ln {dt} M{M}")
    _check(out, ref, bnd, f"quick_gelu gemm_ln {dt} M{M}")


# ---- the read-out ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
@pytest.mark.parametrize("B,L,D,E", [(1, 2, 128, 64), (3, 5, 384, 512), (2, 50, 768, 512)])
def test_head_features_unit_vector_and_similarity(cuda, dt, B, L, D, E):
    g = torch.Generator().manual_seed(B + L + D + E)
    sd = C.random_state_dict(D, 0, 1, E, seed=D + E)
    x_h = 1.5 * torch.randn((B, L, D), generator=g) + 0.4
    x_h[-1, 0] *= 30.0                                                     # a high-norm cls row
    gref = torch.randn(E, generator=g)
    gref = (gref / gref.norm()).contiguous()
    lw, lb, proj = sd["ln_post.weight"].to(cuda), sd["ln_post.bias"].to(cuda), sd["proj"].to(dt).to(cuda)
    run = lambda: clip_ops.head(x_h.to(cuda), lw, lb, proj, gref.to(cuda), C.EPS)
    f, u, s = run()
    f2, u2, s2 = run()
    torch.cuda.synchronize()
    what = f"clip head {dt} B{B} L{L} D{D} E{E}"
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in ((f, f2), (u, u2), (s, s2))), f"{what}: a second launch gave other bits"
    assert f.shape == (B, E) and u.shape == (B, E) and s.shape == (B,)
    fh, uh, sh = f.cpu(), u.cpu(), s.cpu()
    assert torch.equal(fh, fh.to(dt).float()), f"{what}: the features are 16-bit values"
    ref, bnd = C.head_model(x_h[:, 0], sd, dt)
    _check(fh, ref, bnd, what + " features")
    ref, bnd = C.unit_model(fh)
    _check(uh, ref, bnd, what + " unit vector")
    ref, bnd = C.sim_model(uh, gref)
    _check(sh, ref, bnd, what + " similarity")
    nog = clip_ops.head(x_h.to(cuda), lw, lb, proj, None, C.EPS)
    assert nog[2] is None and torch.equal(_bits(nog[0]), _bits(f)) and torch.equal(_bits(nog[1]), _bits(u))


def test_zero_feature_gives_nan_similarity_and_nothing_else(cuda):
    """Image 1's cls row is constant and ln_post has no bias: its centred values, hence h and f, are exactly zero.  Its unit vector and its
    similarity are 0 / 0 = NaN, its features stay zero, and the other images of the batch are untouched."""
    B, L, D, E = 3, 2, 128, 64
    g = torch.Generator().manual_seed(3)
    sd = C.random_state_dict(D, 0, 1, E, seed=1)
    x_h = torch.randn((B, L, D), generator=g)
    x_h[1, 0] = 0.25                                                       # a constant row: centred values are exactly zero
    gref = torch.randn(E, generator=g)
    gref = (gref / gref.norm()).contiguous()
    lw, lb = sd["ln_post.weight"].to(cuda), torch.zeros(D, device=cuda)
    f, u, s = clip_ops.head(x_h.to(cuda), lw, lb, sd["proj"].half().to(cuda), gref.to(cuda), C.EPS)
    assert not f[1].any() and torch.isnan(s[1]) and torch.isnan(u[1]).all()
    assert torch.isfinite(f).all() and torch.isfinite(s[[0, 2]]).all() and torch.isfinite(u[[0, 2]]).all()


# ---- the whole model -----------------------------------------------------------------------------------------------------------------------------
def _model(cuda, D, depth, grid, dt, E=64, seed=0):
    sd = C.random_state_dict(D, depth, grid, E, seed)
    m = CLIPVisionTransformer(input_resolution=grid * 32, patch_size=32, width=D, layers=depth, heads=D // 64, output_dim=E, dtype=dt)
    m.load_state_dict(sd, strict=True)
    return m.to(cuda), sd


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
@pytest.mark.parametrize("D,depth,grid,B", [(128, 2, 2, 3), (384, 2, 3, 2), (768, 1, 7, 2)])
def test_model_against_float64(cuda, dt, D, depth, grid, B):
    """Features: rel-L2 and max-abs deviation from float64 within twice the deviation of the torch composition under CPU autocast at the same
    operand type (the margin every 16-bit route of this project gets).  Similarities of 16 images with a canonical one: the largest deviation of
    the batch within twice the yardstick's largest (a single scalar's yardstick deviation can be arbitrarily small)."""
    m, sd = _model(cuda, D, depth, grid, dt, E=64 if D == 128 else 512, seed=D + grid)
    img = _u8(17, grid, 7)
    ref = C.forward(sd, C.normalise_u8(img, torch.float64))["feat"]
    yard = C.forward_autocast(sd, C.normalise_u8(img), dt).double()
    what = f"CLIP tower D{D} depth{depth} grid{grid} B{B} {dt}"
    h = m.encode_image(img[:B].to(cuda)).cpu().double()
    assert torch.isfinite(h).all()
    e_rel, y_rel = C.rel_l2(h, ref[:B]), C.rel_l2(yard[:B], ref[:B])
    e_max, y_max = float((h - ref[:B]).abs().max()), float((yard[:B] - ref[:B]).abs().max())
    print(f"{what}: HIP / torch-autocast deviation from float64\n  features: rel-L2 {e_rel:.3e} / {y_rel:.3e} = {e_rel / y_rel:.2f}; "
          f"max-abs {e_max:.3e} / {y_max:.3e} = {e_max / y_max:.2f}")
    # 16 pairs (image i, canonical = image 16) in one batched call
    _, canon_unit, _ = m.encode(img[16:].to(cuda))
    sim = m.encode(img[:16].to(cuda), canon_unit[0].contiguous())[2].cpu().double()
    sim64 = C.cosine(ref[:16], ref[16])
    sim_y = C.cosine(yard[:16].float(), yard[16].float()).double()
    s_max, sy_max = float((sim - sim64).abs().max()), float((sim_y - sim64).abs().max())
    print(f"  similarity (16 pairs): max-abs {s_max:.3e} / {sy_max:.3e} = {s_max / sy_max:.2f}")
    assert e_rel <= 2.0 * y_rel and e_max <= 2.0 * y_max, f"{what}: features beyond twice the autocast deviation"
    assert s_max <= 2.0 * sy_max, f"{what}: similarities beyond twice the autocast deviation"


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_batch_position_and_rerun_invariance(cuda, dt):
    D, depth, grid = 384, 2, 3
    m, _ = _model(cuda, D, depth, grid, dt, E=512, seed=31)
    img = _u8(4, grid, 9)
    img[2] = img[0]
    canon = m.encode(img[3:].to(cuda))[1][0].contiguous()
    a = m.encode(img[:3].to(cuda), canon)
    b = m.encode(img[:3].to(cuda), canon)
    solo = m.encode(img[:1].to(cuda), canon)
    for k, name in enumerate(("features", "unit vector", "similarity")):
        assert torch.equal(_bits(a[k]), _bits(b[k])), f"{name}: two runs gave other bits"
        assert torch.equal(_bits(a[k][0]), _bits(a[k][2])), f"{name}: the same image at batch positions 0 and 2 differs"
        assert torch.equal(_bits(a[k][0]), _bits(solo[k][0])), f"{name}: an image's result depends on the batch around it"


@pytest.mark.parametrize("S", [512, 300, 100])
def test_preprocess_equals_pillow(cuda, S):
    pytest.importorskip("PIL.Image")
    img = torch.rand((2, 3, S, S), generator=torch.Generator().manual_seed(S))
    img[0, :, :8] = 1.0                                                    # 255 exactly, and 0
    img[0, :, 8:16] = 0.0
    got = clip_preprocess_u8(img.to(cuda))
    assert got.dtype == torch.uint8 and got.shape == (2, 3, 224, 224)
    assert torch.equal(got.cpu(), C.preprocess_u8(img))


def test_similarity_is_preprocess_encode_cosine(cuda):
    m, sd = _model(cuda, 128, 1, 7, torch.float16, E=64, seed=3)
    g = torch.Generator().manual_seed(4)
    imgs, canon = torch.rand((3, 3, 300, 300), generator=g).to(cuda), torch.rand((3, 300, 300), generator=g).to(cuda)
    s = m.similarity(imgs, canon)
    f = m.encode_image(clip_preprocess_u8(torch.cat([imgs, canon[None]])))
    assert s.shape == (3,) and torch.equal(_bits(s), _bits(m.similarity(imgs, m.unit_feature(canon))))
    want = C.cosine(f[:3].cpu().double(), f[3].cpu().double())
    assert float((s.cpu().double() - want).abs().max()) < 1e-5


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------------
def _untouched(t):
    return bool((t.view(torch.int32) == SENTINEL32).all())


def test_refusals_launch_nothing(cuda):
    D, grid, E = 128, 2, 64
    m, sd = _model(cuda, D, 1, grid, torch.float16, E=E)
    w, cls, pos, lut = _front_args(sd, torch.float16, cuda)
    sent = lambda *shape: torch.full(shape, SENTINEL32, dtype=torch.int32, device=cuda).view(torch.float32)
    # patch embedding: S no multiple of 32, not the grid pos holds, non-square, D no multiple of 128, a table of the other type, wrong pixel type
    for bad, kw in ((torch.zeros((1, 3, 48, 48), dtype=torch.uint8), {}), (torch.zeros((1, 3, 96, 96), dtype=torch.uint8), {}),
                    (torch.zeros((1, 3, 64, 32), dtype=torch.uint8), {}), (torch.zeros((1, 3, 64, 64), dtype=torch.uint8), dict(w=w[:64])),
                    (torch.zeros((1, 3, 64, 64), dtype=torch.uint8), dict(lut=lut.bfloat16())), (torch.zeros((1, 3, 64, 64), dtype=torch.float16), {})):
        out = sent(1, 1 + grid * grid, kw["w"].shape[0] if "w" in kw else D)
        with pytest.raises((_lib.GvfError, AssertionError)):
            clip_ops.patch_embed(bad.to(cuda), kw.get("w", w), cls[:out.shape[-1]].contiguous(), pos[:, :out.shape[-1]].contiguous(),
                                 kw.get("lut", lut), out=out)
        torch.cuda.synchronize()
        assert _untouched(out)
    l = _lib.lib()
    p = lambda t: _lib.ptr(t)
    out = sent(1, 5, D)
    ok_img = torch.zeros((1, 3, 64, 64), dtype=torch.uint8, device=cuda)
    for dtype, kind, S, n, Dv in ((7, 0, 64, 4, D), (1, 2, 64, 4, D), (1, 0, 48, 4, D), (1, 0, 64, 9, D), (1, 0, 64, 4, 64), (1, 0, 64, 4, 192)):
        assert l.gvf_clip_patch_embed(dtype, kind, p(ok_img), p(lut), 1, S, p(w), p(cls), p(pos), n, Dv, p(out), None) == _lib.GVF_EINVAL
    assert l.gvf_clip_patch_embed(1, 0, p(ok_img), None, 1, 64, p(w), p(cls), p(pos), 4, D, p(out), None) == _lib.GVF_EINVAL      # uint8 without a table
    torch.cuda.synchronize()
    assert _untouched(out)
    # ln_pre: widths outside 128 .. 1024 in steps of 128, eps <= 0
    for Dv, eps in ((64, 1e-5), (192, 1e-5), (1152, 1e-5), (128, 0.0)):
        x = sent(3, Dv)
        st = sent(3, max(Dv // 64, 1), 2)
        one = torch.ones(Dv, device=cuda)
        with pytest.raises(_lib.GvfError):
            clip_ops.ln_rows(x, one, one, eps, st)
        torch.cuda.synchronize()
        assert _untouched(x) and _untouched(st)
    # the read-out: E no multiple of 64 or beyond 1024, D beyond 1024, a similarity without its buffer
    for Dv, Ev in ((128, 32), (128, 96), (128, 1088), (1152, 64)):
        outs = (sent(2, Ev), sent(2, Ev), sent(2))
        one = torch.ones(Dv, device=cuda)
        with pytest.raises(_lib.GvfError):
            clip_ops.head(torch.zeros((2, 2, Dv), device=cuda), one, one, torch.zeros((Dv, Ev), dtype=torch.float16, device=cuda),
                          torch.zeros(Ev, device=cuda), C.EPS, out=outs)
        torch.cuda.synchronize()
        assert all(_untouched(o) for o in outs)
    f, u = sent(2, E), sent(2, E)
    one = torch.ones(D, device=cuda)
    assert l.gvf_clip_head(1, p(torch.zeros((2, 2, D), device=cuda)), 2, 2, D, 1e-5, p(one), p(one), p(torch.zeros((D, E), dtype=torch.float16, device=cuda)),
                           E, p(torch.zeros(E, device=cuda)), p(f), p(u), None, None) == _lib.GVF_EINVAL
    torch.cuda.synchronize()
    assert _untouched(f) and _untouched(u)
    # an epilogue code nobody defined
    obuf = _filled((8, 128), torch.float16, cuda)
    a16, w16 = torch.zeros((8, 128), dtype=torch.float16, device=cuda), torch.zeros((128, 128), dtype=torch.float16, device=cuda)
    with pytest.raises(_lib.GvfError):
        dit_ops.gemm(a16, w16, None, obuf, 7)
    torch.cuda.synchronize()
    assert bool((obuf.view(torch.int16) == SENTINEL16).all())
    # the module: CPU tensors, non-square, a side the positional embedding was not stored for
    for bad in (torch.zeros((1, 3, 64, 64), dtype=torch.uint8), torch.zeros((1, 3, 64, 32), dtype=torch.uint8, device=cuda),
                torch.zeros((1, 3, 96, 96), dtype=torch.uint8, device=cuda), torch.zeros((1, 3, 48, 48), dtype=torch.uint8, device=cuda),
                torch.zeros((1, 3, 64, 64), dtype=torch.float64, device=cuda)):
        with pytest.raises(_lib.GvfError):
            m.encode_image(bad)
    with pytest.raises(_lib.GvfError):
        clip_preprocess_u8(torch.zeros((1, 3, 64, 48), device=cuda))
    assert m.encode_image(ok_img).shape == (1, E)


# ---- the alignment seam ----------------------------------------------------------------------------------------------------------------------------
def test_alignment_batched_clip_term_equals_the_per_view_callback(cuda):
    """align_gaussian_to_canonical on a slab with a fin (4 azimuths): clip_model= (one batched encoder call per render chunk) returns the azimuth,
    the scale and, bit for bit, the per-view scores of clip_score= wrapping the same model one image at a time."""
    from gvfdiffusion_amd.attrdict import edict
    from gvfdiffusion_amd.renderers import GaussianRenderer
    from gvfdiffusion_amd.utils.inference_utils import align_gaussian_to_canonical, azimuth_cameras
    P = 6000
    g = torch.Generator().manual_seed(5)
    attrs = synthetic.random_gaussians(P, sh_degree=0, seed=13, scale_lo=0.006, scale_hi=0.015)
    xyz = (torch.rand(P, 3, generator=g) - 0.5) * torch.tensor([0.5, 0.12, 0.35])         # a slab ...
    xyz[: P // 3] = (torch.rand(P // 3, 3, generator=g) - 0.5) * torch.tensor([0.1, 0.3, 0.1]) + torch.tensor([0.2, 0.2, 0.1])  # ... with a fin
    attrs["means3D"] = xyz
    attrs["shs"][: P // 3] = 1.5
    attrs["opacities"] = attrs["opacities"].clamp(min=0.6)
    rend = GaussianRenderer({"resolution": 512, "near": synthetic.NEAR, "far": synthetic.FAR, "bg_color": (1, 1, 1)})
    rend.pipe.kernel_size = synthetic.KERNEL_2D
    K = synthetic.intrinsics().to(cuda)
    vae = SimpleNamespace(renderers=edict({"MipGS": rend}))
    m, _ = _model(cuda, 128, 1, 7, torch.float16, E=64, seed=11)
    gm0 = synthetic.gaussian_model_from(attrs, 0, cuda)
    with torch.no_grad():
        canon = rend.render_frames(gm0, azimuth_cameras([-90]).to(cuda), K, want_alpha_depth=True)
    rgb, alpha = canon.rgb[0].clamp(0, 1), canon.alpha[0]
    calls = []

    def per_view(image, canonical):
        calls.append(1)
        return m.similarity(image[None], canonical)[0]

    runs = []
    for kw in (dict(clip_model=m), dict(clip_score=per_view), {}):
        gm = synthetic.gaussian_model_from(attrs, 0, cuda)
        model, scale, scores = align_gaussian_to_canonical(gm, rgb, alpha, K, vae, id=0, device=cuda, in_the_wild=False, return_scores=True, **kw)
        runs.append((scale, scores, gm.get_xyz.clone()))
    (s_b, sc_b, x_b), (s_c, sc_c, x_c), (s_n, sc_n, x_n) = runs
    assert len(sc_b) == len(sc_c) == len(calls) == 4 and [a for a, _ in sc_b] == [-180, -90, 0, 90]
    assert s_b == s_c and torch.equal(x_b, x_c)
    assert sc_b == sc_c, (sc_b, sc_c)                                       # Python floats: equal means equal bits
    assert all(math.isfinite(d) for _, d in sc_b) and all(b >= n - 1e-6 for (_, b), (_, n) in zip(sc_b, sc_n))      # the CLIP term adds 0.2 (1 - cos) >= 0
    with pytest.raises(ValueError):
        align_gaussian_to_canonical(synthetic.gaussian_model_from(attrs, 0, cuda), rgb, alpha, K, vae, id=0, device=cuda, in_the_wild=False,
                                    clip_model=m, clip_score=per_view)
    assert len(align_gaussian_to_canonical(synthetic.gaussian_model_from(attrs, 0, cuda), rgb, alpha, K, vae, id=0, device=cuda,
                                           in_the_wild=False)) == 2
