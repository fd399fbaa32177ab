"""Conformance of the DINOv2 image encoder on the device (csrc/vit.hip, GVF_EPI_GELU_ERF_16 of csrc/gemm.hip, model/dinov2.py and its callers'
seams) against the float64 restatement of tests/vit_ref.py, which tests/test_vit_ref.py holds to transformers' implementation.

Shapes are the smallest that reach every edge: widths 128 (2 heads) and 384 (6 heads), depth 2, grids 1 x 1 (6 tokens with the 4 registers, 2
without), 3 x 3 (14 tokens) and 5 x 5 (30 tokens: no multiple of any GEMM or attention tile; 75 patches at B = 3: two full 32-patch tiles and
a partial one), B in {1, 3}, R in {0, 4}, fp16 and bf16.  The seams run once at the released geometry (518 x 518, 1374 tokens)
on a width-128 one-block model."""
import math

import pytest
import torch

import gemm_ref as G
import vit_ref as V
from gvfdiffusion_amd import _lib
from gvfdiffusion_amd.model.dinov2 import DinoVisionTransformer
from gvfdiffusion_amd.ops import dit_ops, vit as vit_ops

pytestmark = pytest.mark.gpu
DTYPES = [torch.float16, torch.bfloat16]
IDS = ["fp16", "bf16"]
# (D, grid, B, R)
CONFIGS = [(128, 1, 1, 4), (128, 3, 3, 4), (384, 5, 3, 4), (384, 5, 1, 0), (128, 1, 3, 0)]
SENTINEL16 = 0x7E5A


def _bits(t):
    return t.view(torch.int16) if t.element_size() == 2 else t.view(torch.int32)


def _image(B, grid, seed=0):
    return torch.rand((B, 3, grid * 14, grid * 14), generator=torch.Generator().manual_seed(100 + seed))


def _patch_args(sd, dt, dev):
    D = sd["cls_token"].shape[-1]
    w = vit_ops.pack_patch_weight(sd["patch_embed.proj.weight"].to(dev), dt)
    reg = sd["register_tokens"].reshape(-1, D).contiguous().to(dev) if "register_tokens" in sd else None
    return w, sd["patch_embed.proj.bias"].to(dev), sd["cls_token"].reshape(D).to(dev), reg, sd["pos_embed"].reshape(-1, D).contiguous().to(dev)


def _check(out_h, ref, bnd, what):
    n_bad, worst = G.excess(out_h, ref, bnd)
    print(f"{what}: rel_l2 {V.rel_l2(out_h, ref):.2e}, max |err| / bound {worst:.3f}")
    assert n_bad == 0, f"{what}: {n_bad} of {ref.numel()} elements outside the bound (worst {worst:.2f} x)"


def _model(cuda, D, grid, R, dt, depth=2, seed=0, sd=None):
    sd = V.random_state_dict(D, depth, grid, R, seed) if sd is None else sd
    m = DinoVisionTransformer(img_size=grid * 14, patch_size=14, embed_dim=D, depth=depth, num_heads=D // 64, num_register_tokens=R, dtype=dt)
    m.load_state_dict(sd, strict=True)
    return m.to(cuda), sd


# ---- patch embedding ------------------------------------------------------------------------------------------------------------------------
def _patch_embed_checked(cuda, dt, sd, img, R, what):
    D = sd["cls_token"].shape[-1]
    w, bias, cls, reg, pos = _patch_args(sd, dt, cuda)
    wh = w.cpu()
    assert torch.equal(_bits(wh[:, :V.PATCH_K]), _bits(sd["patch_embed.proj.weight"].reshape(D, -1).to(dt))) and not wh[:, V.PATCH_K:].any()
    x, st = vit_ops.patch_embed(img.to(cuda), w, bias, cls, reg, pos)
    x2, st2 = vit_ops.patch_embed(img.to(cuda), w, bias, cls, reg, pos)
    torch.cuda.synchronize()
    assert torch.equal(_bits(x), _bits(x2)) and torch.equal(_bits(st), _bits(st2)), f"{what}: a second launch gave other bits"
    xh, B = x.cpu(), img.shape[0]
    n = pos.shape[0] - 1
    assert xh.shape == (B, 1 + R + n, D) and st.shape == (B * (1 + R + n), D // 64, 2)
    # cls and register rows: their fp32 definitions, to the bit
    assert torch.equal(xh[:, 0], (sd["cls_token"].reshape(D) + sd["pos_embed"][0, 0]).expand(B, D)), f"{what}: cls row"
    if R:
        assert torch.equal(xh[:, 1:1 + R], sd["register_tokens"].expand(B, R, D)), f"{what}: register rows"
    ref, bnd = V.patch_embed_model(img, sd, dt)
    _check(xh[:, 1 + R:], ref, bnd, what)
    # partial statistics of the rows as stored, per 64-column slice
    parts = D // 64
    rows = xh.reshape(-1, parts, 64).double()
    b_sum, b_sq = G.stats_bound(rows.float())
    sth = st.cpu().double()
    assert bool(((sth[..., 0] - rows.sum(-1)).abs() <= b_sum).all()), f"{what}: row sums"
    assert bool(((sth[..., 1] - (rows * rows).sum(-1)).abs() <= b_sq).all()), f"{what}: row sums of squares"
    return xh


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
@pytest.mark.parametrize("D,grid,B,R", CONFIGS)
def test_patch_embed_elementwise(cuda, dt, D, grid, B, R):
    sd = V.random_state_dict(D, 0, grid, R, seed=D + grid + R)
    _patch_embed_checked(cuda, dt, sd, _image(B, grid, B), R, f"patch_embed {dt} D{D} grid{grid} B{B} R{R}")


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_patch_embed_gather_index(cuda, dt):
    """One hot pixel per (channel, dy, dx) class on a black image, the 588 classes dealt over the 75 patches of three 5 x 5 images: a wrong
    gather index (transposed dy / dx, a channel stride off by one, a neighbouring patch) moves a weight column by far more than the bound."""
    D, grid, B, R = 128, 5, 3, 4
    img = torch.zeros((B, 3, grid * 14, grid * 14))
    for k in range(V.PATCH_K):
        c, dy, dx = k // 196, (k % 196) // 14, k % 14
        p = (k * 7) % (B * grid * grid)
        b, i = divmod(p, grid * grid)
        img[b, c, (i // grid) * 14 + dy, (i % grid) * 14 + dx] = 1.0
    sd = V.random_state_dict(D, 0, grid, R, seed=9)
    _patch_embed_checked(cuda, dt, sd, img, R, f"patch_embed {dt} hot pixels")


# ---- the exact-erf GELU epilogue -------------------------------------------------------------------------------------------------------------
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


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
@pytest.mark.parametrize("M", [6, 30, 90])
def test_gelu_erf_epilogue_gemm(cuda, dt, M):
    N, K = 512, 128
    g = torch.Generator().manual_seed(M)
    a_h = (3.0 * torch.randn((M, K), generator=g)).to(dt)                 # pre-activations of std 3: both erf tails are reached
    w_h = (torch.randn((N, K), generator=g) / math.sqrt(K)).to(dt)
    bias = torch.randn((N,), generator=g)
    bias[::64] = 9.0
    bias[1::64] = -9.0
    obuf = _filled((M + 2, N + 8), dt, cuda)
    a, w, b = a_h.to(cuda), w_h.to(cuda), bias.to(cuda)
    after = _launch_checked(obuf, lambda: dit_ops.gemm(a, w, b, obuf[:M, :N], dit_ops.EPI_GELU_ERF_16), (M, N), f"gelu_erf gemm {dt} M{M}")
    ref, bnd = V.gelu_erf_model(a_h, w_h, bias)
    pre = a_h.double() @ w_h.double().T + bias.double()
    assert float(pre.max()) > 6.0 and float(pre.min()) < -6.0
    _check(after[:M, :N].cpu(), ref, bnd, f"gelu_erf gemm {dt} M{M}")


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
@pytest.mark.parametrize("M", [6, 30, 90])
def test_gelu_erf_epilogue_gemm_ln(cuda, dt, M):
    """The same epilogue behind the LayerNorm-folded operand (the MLP's fc1): statistics from gvf_gemm_resid_stats, as in the model."""
    N, K, Kr = 512, 128, 96
    g = torch.Generator().manual_seed(1000 + M)
    ar_h = torch.randn((M, Kr), generator=g).to(dt)
    wr_h = (torch.randn((K, Kr), generator=g) / math.sqrt(Kr)).to(dt)
    x = (2.0 * torch.randn((M, K), generator=g) + 0.3).to(cuda)
    parts = dit_ops.gemm_stats_parts(K)
    stats = torch.empty((M, parts, 2), device=cuda)
    dit_ops.gemm_resid_stats(ar_h.to(cuda), wr_h.to(cuda), None, x, stats)
    w_h = (3.0 * torch.randn((N, K), generator=g) / math.sqrt(K)).to(dt)
    bias = torch.randn((N,), generator=g)
    bias[::64] = 9.0
    bias[1::64] = -9.0
    ln_w, ln_b = 1.0 + 0.2 * torch.randn(K, generator=g), 0.2 * torch.randn(K, generator=g)
    obuf = _filled((M + 2, N + 8), dt, cuda)
    w, b, lw, lb = w_h.to(cuda), bias.to(cuda), ln_w.to(cuda), ln_b.to(cuda)
    after = _launch_checked(obuf, lambda: dit_ops.gemm_ln_bf16(x, stats, parts, w, b, obuf[:M, :N], dit_ops.EPI_GELU_ERF_16, eps=1e-6, ln_w=lw, ln_b=lb),
                            (M, N), f"gelu_erf gemm_ln {dt} M{M}")
    a16, amb = G.ln_operand(x.cpu(), parts, dt, 1e-6, ln_w, ln_b)
    ref, bnd = V.gelu_erf_model(a16, w_h, bias, a_err=amb.abs() @ w_h.double().abs().T)
    pre = a16.double() @ w_h.double().T + bias.double()
    assert float(pre.max()) > 6.0 and float(pre.min()) < -6.0
    _check(after[:M, :N].cpu(), ref, bnd, f"gelu_erf gemm_ln {dt} M{M}")


# ---- the read-out ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,R,n,D", [(3, 4, 25, 384), (1, 0, 1, 128), (2, 4, 9, 1024)])
def test_tokens_out_modes_orders_types(cuda, B, R, n, D):
    g = torch.Generator().manual_seed(B + R + n + D)
    x_h = 1.5 * torch.randn((B, 1 + R + n, D), generator=g) + 0.4
    x_h[:, -1] *= 30.0                                                    # a high-norm row
    ln_w, ln_b = 1.0 + 0.2 * torch.randn(D, generator=g), 0.2 * torch.randn(D, generator=g)
    x, lw, lb = x_h.to(cuda), ln_w.to(cuda), ln_b.to(cuda)
    for odt in (torch.float32, torch.float16):
        for mode in (vit_ops.OUT_COPY, vit_ops.OUT_LN_AFFINE, vit_ops.OUT_LN):
            kw = dict(ln_w=lw, ln_b=lb) if mode == vit_ops.OUT_LN_AFFINE else {}
            stored = vit_ops.tokens_out(x, R, mode, vit_ops.ORDER_STORED, odt, **kw)
            cond = vit_ops.tokens_out(x, R, mode, vit_ops.ORDER_PATCHES_CLS, odt, **kw)
            again = vit_ops.tokens_out(x, R, mode, vit_ops.ORDER_STORED, odt, **kw)
            torch.cuda.synchronize()
            what = f"tokens_out B{B} R{R} n{n} D{D} mode{mode} {odt}"
            assert stored.dtype == odt and stored.shape == (B, 1 + R + n, D) and cond.shape == (B, n + 1, D)
            assert torch.equal(_bits(stored), _bits(again)), f"{what}: a second launch gave other bits"
            assert torch.equal(_bits(cond), _bits(V.cond_layout(stored, R))), f"{what}: patches-then-cls is not a row permutation of the stored order"
            if mode == vit_ops.OUT_COPY:
                ref, bnd = x_h.double(), G._round_bound(x_h.double(), torch.zeros((), dtype=torch.float64), None if odt == torch.float32 else odt)
            elif mode == vit_ops.OUT_LN_AFFINE:
                ref, bnd = V.layernorm_model(x_h, 1e-6, ln_w, ln_b, None if odt == torch.float32 else odt)
            else:
                ref, bnd = V.layernorm_model(x_h, 1e-5, None, None, None if odt == torch.float32 else odt)
            _check(stored.cpu(), ref, bnd, what)


# ---- the whole model -----------------------------------------------------------------------------------------------------------------------------
def _hip_readouts(m, img):
    from gvfdiffusion_amd.trellis.pipelines import encode_image
    out = m(img, is_training=True)
    R = m.num_register_tokens
    assert out["x_norm_clstoken"].shape == (img.shape[0], m.embed_dim) and out["x_norm_regtokens"].shape[1] == R
    x_norm = torch.cat([out["x_norm_clstoken"][:, None], out["x_norm_regtokens"], out["x_norm_patchtokens"]], 1)
    return {"x_prenorm": out["x_prenorm"].cpu(), "x_norm": x_norm.cpu(), "trellis": encode_image(m, img).cpu()}


def _against_yardstick(hip, ref, yard, R, what):
    """x_prenorm, x_norm_patchtokens and the TRELLIS read-out: rel-L2 and max-abs deviation from float64 within twice the deviation of the torch
    composition under CPU autocast at the same operand type (the margin every 16-bit route of this project gets: summation order differs)."""
    bad, rows = [], []
    for k, sl in (("x_prenorm", slice(None)), ("x_norm", slice(R + 1, None)), ("trellis", slice(None))):
        h, r, y = hip[k][:, sl].double(), ref[k][:, sl], yard[k][:, sl].double()
        assert torch.isfinite(h).all()
        e_rel, y_rel = V.rel_l2(h, r), V.rel_l2(y, r)
        e_max, y_max = float((h - r).abs().max()), float((y - r).abs().max())
        rows.append(f"  {k}: rel-L2 {e_rel:.3e} / {y_rel:.3e} = {e_rel / y_rel:.2f}; max-abs {e_max:.3e} / {y_max:.3e} = {e_max / y_max:.2f}")
        if not (e_rel <= 2.0 * y_rel and e_max <= 2.0 * y_max):
            bad.append(rows[-1])
    print(f"{what}: HIP / torch-autocast deviation from float64\n" + "\n".join(rows))
    assert not bad, f"{what}: beyond twice the autocast deviation:\n" + "\n".join(bad)


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
@pytest.mark.parametrize("D,grid,B,R", CONFIGS[:4])
def test_model_against_float64(cuda, dt, D, grid, B, R):
    m, sd = _model(cuda, D, grid, R, dt, seed=D + grid)
    img = _image(B, grid, 7)
    hip = _hip_readouts(m, img.to(cuda))
    _against_yardstick(hip, V.forward(sd, img, R), V.forward_autocast(sd, img, R, dt), R, f"ViT D{D} grid{grid} B{B} R{R} {dt}")


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_model_with_high_norm_patch_tokens(cuda, dt):
    """Three patch tokens (the first, a middle one, the last) carry 8 x the typical norm through their position rows -- the artefact tokens a
    DINOv2 backbone is known for (synthetic.dit_inputs_hostile gives the DiT's conditions the same treatment)."""
    D, grid, B, R = 384, 5, 3, 4
    sd = V.random_state_dict(D, 2, grid, R, seed=21)
    g = torch.Generator().manual_seed(22)
    for i in (0, 12, 24):
        sd["pos_embed"][0, 1 + i] += 8.0 * torch.randn(D, generator=g)
    m, _ = _model(cuda, D, grid, R, dt, sd=sd)
    img = _image(B, grid, 8)
    _against_yardstick(_hip_readouts(m, img.to(cuda)), V.forward(sd, img, R), V.forward_autocast(sd, img, R, dt), R, f"ViT high-norm tokens {dt}")


# ---- invariants ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_batch_position_and_rerun_invariance(cuda, dt):
    D, grid, R = 384, 5, 4
    m, _ = _model(cuda, D, grid, R, dt, seed=31)
    img = _image(3, grid, 9)
    img[2] = img[0]
    a = _hip_readouts(m, img.to(cuda))
    b = _hip_readouts(m, img.to(cuda))
    solo = _hip_readouts(m, img[:1].to(cuda))
    for k in a:
        assert torch.equal(_bits(a[k]), _bits(b[k])), f"{k}: two runs gave other bits"
        assert torch.equal(_bits(a[k][0]), _bits(a[k][2])), f"{k}: the same image at batch positions 0 and 2 differs"
        assert torch.equal(_bits(a[k][0]), _bits(solo[k][0])), f"{k}: an image's tokens depend on the batch around it"


def test_refusals_launch_nothing(cuda):
    D, grid, R = 128, 3, 4
    m, sd = _model(cuda, D, grid, R, torch.float16, depth=1)
    w, bias, cls, reg, pos = _patch_args(sd, torch.float16, cuda)
    ok = _image(1, grid).to(cuda)
    for bad in (torch.rand((1, 3, 43, 42), device=cuda), torch.rand((1, 3, 42, 45), device=cuda),      # H / W no multiple of 14
                torch.rand((1, 3, 28, 28), device=cuda), torch.rand((1, 3, 42, 56), device=cuda)):     # not the grid pos_embed holds
        with pytest.raises(_lib.GvfError):
            vit_ops.patch_embed(bad, w, bias, cls, reg, pos)
        with pytest.raises(_lib.GvfError):
            m(bad)
    with pytest.raises(_lib.GvfError):
        vit_ops.patch_embed(ok.cpu(), w, bias, cls, reg, pos)
    with pytest.raises(_lib.GvfError):
        m(ok.cpu())
    with pytest.raises(_lib.GvfError):
        vit_ops.tokens_out(torch.zeros((1, 6, 128)), R)
    with pytest.raises(_lib.GvfError):
        vit_ops.pack_patch_weight(sd["patch_embed.proj.weight"])
    with pytest.raises(_lib.GvfError):                                     # width beyond the read-out's registers
        vit_ops.tokens_out(torch.zeros((1, 6, 1152), device=cuda), R)
    assert m(ok)["x_prenorm"].shape == (1, 1 + R + grid * grid, D)


# ---- the callers' seams, once at the released geometry (518 x 518: 1374 tokens) --------------------------------------------------------------
@pytest.fixture(scope="module")
def released_geometry(cuda):
    m, sd = _model(cuda, 128, 37, 4, torch.float16, depth=1, seed=41)
    return m, sd


def test_encode_image_uint8_equals_pillow_path(cuda, released_geometry):
    Image = pytest.importorskip("PIL.Image")
    import numpy as np
    from gvfdiffusion_amd.trellis.pipelines import encode_image, get_cond
    m, _ = released_geometry
    g = torch.Generator().manual_seed(51)
    yy, xx = torch.meshgrid(torch.arange(300.0), torch.arange(400.0), indexing="ij")
    frames = torch.stack([(127.0 + 90.0 * torch.sin(xx / (7.0 + c) + f) * torch.cos(yy / (11.0 - c)) + 20.0 * torch.randn((300, 400), generator=g))
                          .clamp(0, 255).to(torch.uint8) for f in range(2) for c in range(3)]).view(2, 3, 300, 400).permute(0, 2, 3, 1).contiguous()
    pil = [np.array(Image.fromarray(f.numpy()).resize((518, 518), Image.LANCZOS).convert("RGB")).astype(np.float32) / 255 for f in frames]
    tensor = torch.stack([torch.from_numpy(i).permute(2, 0, 1).float() for i in pil]).to(cuda)
    a, b = encode_image(m, frames.to(cuda)), encode_image(m, tensor)
    assert a.shape == (2, 1374, 128) and a.dtype == torch.float32 and torch.equal(a, b)
    c = get_cond(m, tensor)
    assert torch.equal(c["cond"], b) and not c["neg_cond"].any() and c["neg_cond"].shape == b.shape


def test_encode_cond_frames_is_the_scripts_slicing(cuda, released_geometry):
    from gvfdiffusion_amd.utils import encode_cond_frames
    m, _ = released_geometry
    R = m.num_register_tokens
    img = torch.rand((2, 3, 518, 518), generator=torch.Generator().manual_seed(52)).to(cuda)
    f = m(img, is_training=True)
    raw = torch.cat([f["x_prenorm"][:, R + 1:], f["x_prenorm"][:, :1]], 1).half()
    norm = torch.cat([f["x_norm_patchtokens"], f["x_norm_clstoken"][:, None]], 1).half()
    a, b = encode_cond_frames(m, img), encode_cond_frames(m, img, normalize=True)
    assert a.shape == (2, 1370, 128) and a.dtype == torch.float16
    assert torch.equal(_bits(a), _bits(raw)) and torch.equal(_bits(b), _bits(norm))


def test_image_to_gaussians_equals_its_two_halves(cuda):
    import json
    import os
    import numpy as np
    import slat_flow_ref as SF
    import sparse_structure_ref as SR
    from gvfdiffusion_amd.trellis import models as tm
    from gvfdiffusion_amd.trellis.pipelines import encode_image, image_to_gaussians, tokens_to_gaussians
    z = np.load(os.path.join(os.path.dirname(__file__), "golden", "slat_decoder_golden.npz"))
    cfg = json.loads(bytes(z["cfg_json"]).decode())
    torch.manual_seed(3)
    gs = tm.SLatGaussianDecoder(**cfg)
    torch.nn.init.normal_(gs.out_layer.weight, std=0.02)
    flow_cfg, slat_cfg = dict(SR.FLOW_SMALL["p1"], cond_channels=128), dict(SF.SMALL, cond_channels=128)
    models = {"sparse_structure_flow_model": SR.load_weights(SR.build_flow(flow_cfg), 3), "sparse_structure_decoder": SR.load_weights(SR.build_decoder(SR.DEC_SMALL), 4),
              "slat_flow_model": SF.load_weights(SF.build(slat_cfg), SF.make_weights(slat_cfg, 3))}
    for m in models.values():
        m.to(cuda).set_compute_dtype(torch.float16)
    models["slat_decoder_gs"] = gs.to(cuda)
    models["image_cond_model"], _ = _model(cuda, 128, 3, 4, torch.float16, seed=61)
    img = _image(2, 3, 11).to(cuda)
    noise = SR.flow_inputs("p1")[0].to(cuda)
    norm = dict(mean=[0.05 * i for i in range(8)], std=[1.0 + 0.1 * i for i in range(8)])
    torch.manual_seed(11)
    reps, slat, coords = image_to_gaussians(models, img, 2, SR.PIPE_PARAMS, SR.PIPE_PARAMS, norm, noise=noise)
    cond = encode_image(models["image_cond_model"], img)
    torch.manual_seed(11)
    reps2, slat2, coords2 = tokens_to_gaussians(models, cond, torch.zeros_like(cond), 2, SR.PIPE_PARAMS, SR.PIPE_PARAMS, norm, noise=noise)
    torch.cuda.synchronize()
    assert coords.shape[0] >= 1 and torch.equal(coords, coords2) and torch.equal(slat.feats, slat2.feats) and len(reps) == len(reps2) == 2
    for a, b in zip(reps, reps2):
        assert torch.isfinite(a.get_xyz).all() and torch.equal(a.get_xyz, b.get_xyz) and torch.equal(a.get_opacity, b.get_opacity)
