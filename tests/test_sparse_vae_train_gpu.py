"""The static VAE trains on the HIP operators: one block, the whole backbone, SparseVAE.training_losses and a train_step, against float64
autograd of oracle/sparse_vae_ref.py.  The unit of every bar is the "yardstick": the same oracle with its `precision` set to the operand type
(fp32 arithmetic, 16-bit roundings where the HIP path rounds), measured against the float64 run; the kernels get twice its deviation."""
import pytest
import torch

import sparse_train_ref as R
from test_sparse_vae_gpu import TOL16, TOL16_FP16, _voxels

pytestmark = pytest.mark.gpu
DTYPES = [(torch.bfloat16, "bf16"), (torch.float16, "fp16")]
_CACHE = {}


def _cached(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


# ---- one block ------------------------------------------------------------------------------------------------------------------------
C, H = 128, 2
MODES = {"full": dict(attn_mode="full"), "windowed": dict(attn_mode="windowed", window_size=8, shift_window=4),
         "serialized": dict(attn_mode="serialized", window_size=1024)}


def _block_inputs():
    g = torch.Generator().manual_seed(21)
    coords = _voxels(16, (150, 90), 5)
    x = torch.randn((coords.shape[0], C), generator=g)
    w = torch.randn((coords.shape[0], C), generator=g)
    shapes = {"attn.to_qkv.weight": (3 * C, C), "attn.to_qkv.bias": (3 * C,), "attn.to_out.weight": (C, C), "attn.to_out.bias": (C,),
              "mlp.mlp.0.weight": (4 * C, C), "mlp.mlp.0.bias": (4 * C,), "mlp.mlp.2.weight": (C, 4 * C), "mlp.mlp.2.bias": (C,)}
    sd = {k: torch.randn(s, generator=g) * (s[1] ** -0.5 if len(s) == 2 else 0.1) for k, s in shapes.items()}
    for k in ("attn.q_rms_norm.gamma", "attn.k_rms_norm.gamma"):
        sd[k] = 1 + 0.1 * torch.randn((H, C // H), generator=g)
    return coords, x, w, sd


def _oracle_block(coords, x, w, sd, gid, precision, old, rms, dtype):
    from oracle import sparse_vae_ref as ref
    keys = [k for k in sd if rms or "rms_norm" not in k]
    leaves = {"b." + k: sd[k].to(dtype).requires_grad_() for k in keys}
    xi = x.to(dtype).requires_grad_()
    y = ref.block(xi, gid, leaves, "b", H, precision, old, rms)
    grads = torch.autograd.grad((y * w.to(dtype)).sum(), [leaves["b." + k] for k in keys] + [xi])
    out = dict(zip(keys + ["x"], grads))
    out["y"] = y.detach()
    return out


@pytest.mark.parametrize("dt,name", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("rms", [False, True], ids=["plain", "qk_rms"])
@pytest.mark.parametrize("old", [True, False], ids=["old_layout", "new_layout"])
@pytest.mark.parametrize("mode", list(MODES))
def test_block_output_and_every_gradient(cuda, mode, old, rms, dt, name):
    """128 channels, 2 heads, 150 + 90 voxels on a 16^3 grid.  `serialized` with the default window (one sequence a sample) is full
    attention in another token order, so the oracle's groups are the samples; several windows a sample are the next test's."""
    from gvfdiffusion_amd import sparse as sp
    from gvfdiffusion_amd.model.sparse_voxel_diffusion import SparseTransformerBlock
    from oracle import sparse_vae_ref as ref
    coords, x, w, sd = _cached("block_inputs", _block_inputs)
    gid = ref.window_ids(coords, 8, 4) if mode == "windowed" else coords[:, 0].long()
    r64 = _cached(("b64", mode, old, rms), lambda: _oracle_block(coords, x, w, sd, gid, "fp32", old, rms, torch.float64))
    yard = _oracle_block(coords, x, w, sd, gid, name, old, rms, torch.float32)
    blk = SparseTransformerBlock(C, num_heads=H, modulated=False, use_old_attn_impl=old, qk_rms_norm=rms, **MODES[mode])
    blk.load_state_dict({k: v for k, v in sd.items() if rms or "rms_norm" not in k})
    blk = blk.cuda()
    st = sp.SparseTensor(x.cuda(), coords.cuda())
    xr = x.cuda().requires_grad_()
    y = blk.forward_rows_train(xr, st, dt, cache={})
    names, params = zip(*blk.named_parameters())
    grads = dict(zip(names + ("x",), torch.autograd.grad((y * w.cuda()).sum(), list(params) + [xr])))
    grads["y"] = y.detach()
    log = []
    for k in sorted(r64):
        e, ey = R.rel_l2(grads[k].cpu(), r64[k]), R.rel_l2(yard[k], r64[k])
        log.append(f"{k} {e:.2e}/{ey:.2e}")
        assert torch.isfinite(grads[k]).all() and e <= 2 * ey, f"{mode} old={old} rms={rms} {name} {k}: rel L2 {e:.3e} > 2 x yardstick {ey:.3e}"
    print(f"block {mode} old={old} rms={rms} {name} | kernel/yardstick:", "; ".join(log))


@pytest.mark.parametrize("dt,name", DTYPES, ids=["bf16", "fp16"])
def test_block_serialized_with_several_windows_a_sample(cuda, dt, name):
    """Windows of 64 tokens over 150 + 90 voxels: the serialisation index repeats rows, so gather_rows takes torch's index_add_ for its
    gradient.  The oracle has no overlapping groups; the reference is the same wiring through TorchOps in float64 on the CPU over the
    partition computed on the device (TorchOps is held to the oracle by tests/test_sparse_train_host.py), the yardstick TorchOps with the
    operand type at its stores."""
    from gvfdiffusion_amd import sparse as sp
    from gvfdiffusion_amd.model.sparse_voxel_diffusion import SparseTransformerBlock
    from gvfdiffusion_amd.model.sparse_voxel_diffusion.sparse_transformer import token_partition
    coords, x, w, sd = _cached("block_inputs", _block_inputs)
    sd = {k: v for k, v in sd.items() if "rms_norm" not in k}
    blk = SparseTransformerBlock(C, num_heads=H, attn_mode="serialized", window_size=64, modulated=False, use_old_attn_impl=False)
    blk.load_state_dict(sd)
    st = sp.SparseTensor(x.cuda(), coords.cuda())
    a = blk.attn
    fwd, bwd, cu, longest = token_partition(st, a.attn_mode, a.window_size, a.shift_sequence, a.shift_window, a.serialize_mode)
    assert fwd.numel() > x.shape[0] and bwd.numel() == x.shape[0]
    key = f"rows_{a.attn_mode}_{a.window_size}_{a.shift_sequence}_{a.shift_window}_{a.serialize_mode}"

    def through_torch(dtype, lp):
        b = SparseTransformerBlock(C, num_heads=H, attn_mode="serialized", window_size=64, modulated=False, use_old_attn_impl=False)
        b.load_state_dict(sd)
        b = b.to(dtype)
        stc = sp.SparseTensor(x.to(dtype), coords)
        stc.register_spatial_cache(key, (fwd.cpu(), bwd.cpu(), cu.cpu(), longest))
        xi = x.to(dtype).requires_grad_()
        y = b.forward_rows_train(xi, stc, lp, ops=R.TorchOps())
        names, params = zip(*b.named_parameters())
        out = dict(zip(names + ("x",), torch.autograd.grad((y * w.to(dtype)).sum(), list(params) + [xi])))
        out["y"] = y.detach()
        return out
    r64, yard = through_torch(torch.float64, torch.float64), through_torch(torch.float32, dt)
    blk = blk.cuda()
    xr = x.cuda().requires_grad_()
    y = blk.forward_rows_train(xr, st, dt, cache={})
    names, params = zip(*blk.named_parameters())
    grads = dict(zip(names + ("x",), torch.autograd.grad((y * w.cuda()).sum(), list(params) + [xr])))
    grads["y"] = y.detach()
    log = []
    for k in sorted(r64):
        e, ey = R.rel_l2(grads[k].cpu(), r64[k]), R.rel_l2(yard[k], r64[k])
        log.append(f"{k} {e:.2e}/{ey:.2e}")
        assert e <= 2 * ey, f"serialized x several windows {name} {k}: rel L2 {e:.3e} > 2 x yardstick {ey:.3e}"
    print(f"block serialized, windows of 64, {name} | kernel/yardstick:", "; ".join(log))


# ---- the backbone ---------------------------------------------------------------------------------------------------------------------
def _gold():
    return _cached("gold", R.golden)


def _ref64():
    return _cached("ref64", lambda: R.golden_loss(*_gold()))


def _gpu_model(cfg, sd, dt, **kw):
    from gvfdiffusion_amd.model.sparse_voxel_diffusion import SparseTransformerVAE
    m = SparseTransformerVAE(**dict(cfg, **kw))
    m.load_state_dict(sd, strict=True)
    return m.cuda().enable_training(dtype=dt)


def _gpu_grads(m, feats, coords, noise, W, scale=1.0):
    from gvfdiffusion_amd import sparse as sp
    x = sp.SparseTensor(feats.cuda().requires_grad_(), coords.cuda())
    loss, out = R.model_loss(m, x, noise.cuda(), W.cuda())
    names, params = zip(*m.named_parameters())
    g = torch.autograd.grad(loss * scale, list(params) + [x.feats])
    return loss.detach(), out.feats.detach(), {k: v / scale for k, v in zip(names + ("feats",), g)}


@pytest.mark.parametrize("dt,name", DTYPES, ids=["bf16", "fp16"])
def test_backbone_gradients_at_the_golden_config(cuda, dt, name):
    """loss = sum(out * W) / T + kl at the golden config (fp16 with a loss scale of 1024).  Per tensor max(2 x yardstick, 1e-5), the whole
    gradient 2 x the yardstick's whole-gradient figure.  Yardsticks measured on the CPU: bf16 2.3e-3 .. 6.2e-3 per tensor, 4.1e-3 whole;
    fp16 3.1e-4 .. 7.9e-4, 5.3e-4 whole; out_layer.bias 1.2e-7 (no 16-bit rounding reaches a column sum of the upstream gradient), the only
    tensor on the 1e-5 floor."""
    from gvfdiffusion_amd import sparse as sp
    cfg, sd, feats, coords, noise, W = _gold()
    loss64, out64, g64 = _ref64()
    _, _, gy = R.golden_loss(cfg, sd, feats, coords, noise, W, precision=name, dtype=torch.float32)
    m = _gpu_model(cfg, sd, dt)
    scale = 1024.0 if dt == torch.float16 else 1.0
    loss, out, g = _gpu_grads(m, feats, coords, noise, W, scale)
    assert set(g) == set(g64)
    floor, log = [], []
    for k in sorted(g64):
        assert float(g64[k].abs().max()) > 0, f"{k}: zero reference gradient"
        e, ey = R.rel_l2(g[k].cpu(), g64[k]), R.rel_l2(gy[k], g64[k])
        log.append(f"{k} {e:.2e}/{ey:.2e}")
        if 2 * ey < 1e-5:
            floor.append(k)
        assert torch.isfinite(g[k]).all() and e <= max(2 * ey, 1e-5), f"{name} {k}: rel L2 {e:.3e} > max(2 x {ey:.3e}, 1e-5)"
    assert floor == ["out_layer.bias"], floor
    keys = sorted(g64)
    cat = lambda d: torch.cat([d[k].detach().cpu().double().reshape(-1) for k in keys])   # noqa: E731
    e, ey = R.rel_l2(cat(g), cat(g64)), R.rel_l2(cat(gy), cat(g64))
    print(f"backbone {name} | kernel/yardstick:", "; ".join(log), f"| whole {e:.2e}/{ey:.2e}")
    assert e <= 2 * ey, f"{name}: whole gradient {e:.3e} > 2 x yardstick {ey:.3e}"
    # the same bits on a second run and under use_checkpoint
    _, out2, g2 = _gpu_grads(m, feats, coords, noise, W, scale)
    mc = _gpu_model(cfg, sd, dt, use_checkpoint=True)
    _, outc, gc = _gpu_grads(mc, feats, coords, noise, W, scale)
    assert torch.equal(out, out2) and torch.equal(out, outc)
    for k in g:
        assert torch.equal(g[k], g2[k]), f"{k}: a second run gave other bits"
        assert torch.equal(g[k], gc[k]), f"{k}: use_checkpoint gave other bits"
    # switch off, or no_grad: the inference path, bit for bit; the training output agrees with it within TOL16
    from gvfdiffusion_amd.model.sparse_voxel_diffusion import SparseTransformerVAE
    plain = SparseTransformerVAE(**cfg)
    plain.load_state_dict(sd, strict=True)
    plain = plain.cuda().set_compute_dtype(dt)
    x = sp.SparseTensor(feats.cuda(), coords.cuda())
    z0, mean0, lv0 = plain.encode(x, sample_posterior=False, return_raw=True)
    y0 = plain.decode(z0)
    m.set_compute_dtype(dt)
    with torch.no_grad():
        z1, mean1, lv1 = m.encode(x, sample_posterior=False, return_raw=True)
        y1 = m.decode(z1)
    m.enable_training(False)
    z2, mean2, lv2 = m.encode(x, sample_posterior=False, return_raw=True)
    y2 = m.decode(z2)
    for a, b, c in ((mean0, mean1, mean2), (lv0, lv1, lv2), (y0.feats, y1.feats, y2.feats)):
        assert torch.equal(a, b) and torch.equal(a, c) and not b.requires_grad and not c.requires_grad
    m.enable_training(dtype=dt)
    zt, meant, lvt = m.encode(x, sample_posterior=False, return_raw=True)
    yt = m.decode(z0)
    assert meant.grad_fn is not None and yt.feats.grad_fn is not None and yt.feats.dtype == torch.float32
    tol = TOL16_FP16 if dt == torch.float16 else TOL16
    for a, b, what in ((meant, mean0, "mean"), (lvt, lv0, "logvar"), (yt.feats, y0.feats, "decode")):
        e = R.rel_l2(a.detach(), b)
        print(f"training vs inference output, {what} [{name}]: rel L2 {e:.2e}")
        assert e < tol, (what, e)


# ---- training_losses ------------------------------------------------------------------------------------------------------------------
REP_CFG = {"MipGS": {"lr": {"_xyz": 1.0, "_features_dc": 1.0, "_opacity": 1.0, "_scaling": 1.0, "_rotation": 0.1}, "perturb_offset": True,
                     "reg_mode": "soft_invoxel", "voxel_size": 1.5, "num_gaussians": 8, "2d_filter_kernel_size": 0.1,
                     "3d_filter_kernel_size": 0.0009, "scaling_bias": 0.004, "opacity_bias": 0.1, "scaling_activation": "softplus"}}
# chosen so that every term carries at least 1 % of the gradient (asserted below): the weights a wiring error would have to hide behind
# (measured shares on to_latent with lambda_lpips = 0.2: l1 1.20, ssim 0.26, lpips 0.0007, kl 0.18, vol 0.13, opacity 0.16 -- the seeded random
# LPIPS weights give a small term, hence its weight of 20)
LAMBDAS = dict(lambda_ssim=0.2, lambda_lpips=20.0, lamda_kl=1e-3, lambda_vol=1e4, lambda_opacity=1e-2)


def _framework(dt):
    from gvfdiffusion_amd import sparse as sp
    from gvfdiffusion_amd.model.sparse_voxel_diffusion import SparseVAE
    from gvfdiffusion_amd.ops.lpips import LPIPS
    from gvfdiffusion_amd.synthetic import camera_block
    cfg, sd, feats, coords, noise, W = _gold()
    m = _gpu_model(cfg, sd, dt)
    vae = SparseVAE({"vae": m}, resolution=cfg["resolution"], representation_config=REP_CFG, loss_type="l1", lambda_ssim=LAMBDAS["lambda_ssim"],
                    lambda_lpips=LAMBDAS["lambda_lpips"], lamda_kl=LAMBDAS["lamda_kl"],
                    regularizations={"MipGS": {"lambda_vol": LAMBDAS["lambda_vol"], "lambda_opacity": LAMBDAS["lambda_opacity"]}})
    cams = [camera_block(azi=30.0, elev=15.0), camera_block(azi=200.0, elev=-10.0)]
    ext = torch.stack([c["extrinsics"] for c in cams]).cuda()
    intr = torch.stack([c["intrinsics"] for c in cams]).cuda()
    g = torch.Generator().manual_seed(8)
    image = torch.nn.functional.interpolate(torch.rand((2, 3, 8, 8), generator=g), size=(64, 64), mode="bilinear", align_corners=False).cuda()
    lp = LPIPS().cuda()                                               # seeded pseudo-random weights: nothing is downloaded
    x = sp.SparseTensor(feats.cuda(), coords.cuda())
    return vae, m, x, image, ext, intr, lp, noise.cuda()


def test_training_losses_terms_and_gradient(cuda):
    import ssim_ref
    vae, m, x, image, ext, intr, lp, noise = _framework(torch.bfloat16)
    terms, reps, aux = vae.training_losses(x, image, ext, intr, return_aux=True, lpips=lp, noise=noise)
    assert set(terms) == {"loss", "rec", "MipGS_l1", "MipGS_ssim", "MipGS_lpips", "kl", "reg_MipGS_vol", "reg_MipGS_opacity"}
    assert aux["rec_image"].shape == (2, 3, 64, 64) and len(reps["MipGS"]) == 2
    # kl and the regularisers: their float64 formulas on the returned tensors, within the derived bounds
    h = torch.cat([aux["mean"], aux["logvar"]], dim=1).detach().cpu()
    L = aux["mean"].shape[1]
    kl64 = R.posterior(h, torch.zeros((h.shape[0], L)), torch.zeros((h.shape[0], L)), 0.0)["kl"]
    assert abs(float(terms["kl"]) - float(kl64)) <= R.kl_bound(h, L)
    s = torch.cat([r._scaling for r in reps["MipGS"]]).detach().cpu()
    o = torch.cat([r._opacity for r in reps["MipGS"]]).detach().cpu()
    g0 = reps["MipGS"][0]
    consts = (float(g0.scale_bias), float(g0.opacity_bias), g0.mininum_kernel_size, True)
    r64 = R.reg(s, o, *consts, 0.0, 0.0)
    bv, bo = R.reg_bounds(s, o, *consts)
    assert abs(float(terms["reg_MipGS_vol"]) - float(r64["vol"])) <= bv and abs(float(terms["reg_MipGS_opacity"]) - float(r64["opa"])) <= bo
    # l1 and ssim: tests/ssim_ref.py on the rendered images, the bar of tests/test_image_loss_gpu.py (twice the fp32 torch composition, floor 1e-7)
    rec, gt = aux["rec_image"].detach().cpu(), aux["gt_image"].cpu()
    l1_64, s64 = float((rec.double() - gt.double()).abs().mean()), float(ssim_ref.ssim64(rec, gt))
    e32 = abs(float(ssim_ref.ssim_torch32(rec, gt)) - s64)
    assert abs(float(terms["MipGS_l1"]) - l1_64) <= max(2 * abs(float(torch.nn.functional.l1_loss(rec, gt)) - l1_64), 1e-7)
    assert abs(float(terms["MipGS_ssim"]) - (1 - s64)) <= max(2 * e32, 1e-7)
    # loss: the weighted sum of its terms
    want = float(terms["MipGS_l1"]) + LAMBDAS["lambda_ssim"] * float(terms["MipGS_ssim"]) + LAMBDAS["lambda_lpips"] * float(terms["MipGS_lpips"]) + \
        LAMBDAS["lamda_kl"] * float(terms["kl"]) + LAMBDAS["lambda_vol"] * float(terms["reg_MipGS_vol"]) + \
        LAMBDAS["lambda_opacity"] * float(terms["reg_MipGS_opacity"])
    assert abs(float(terms["loss"]) - want) <= 1e-6 * abs(want)
    # every term's share of the gradient, on the encoder's last projection (to_latent): the last parameters EVERY term reaches -- the KL
    # term does not pass through the decoder rows.  One backward per term.
    weighted = {"MipGS_l1": 1.0, "MipGS_ssim": LAMBDAS["lambda_ssim"], "MipGS_lpips": LAMBDAS["lambda_lpips"], "kl": LAMBDAS["lamda_kl"],
                "reg_MipGS_vol": LAMBDAS["lambda_vol"], "reg_MipGS_opacity": LAMBDAS["lambda_opacity"]}
    # (a fresh forward per term: the LPIPS operator frees its saved activations in its backward, so its graph is walked once)
    names, params = zip(*m.named_parameters())
    got = torch.autograd.grad(terms["loss"], params)
    on = [names.index("to_latent.weight"), names.index("to_latent.bias")]
    cat = lambda gs: torch.cat([g.reshape(-1) for g in gs])   # noqa: E731
    total = cat([got[i] for i in on]).norm()
    shares = {}
    for k, lam in weighted.items():
        t2, _ = vae.training_losses(x, image, ext, intr, lpips=lp, noise=noise)
        gk = torch.autograd.grad(t2[k], [params[i] for i in on], allow_unused=True)
        shares[k] = float(lam * cat([torch.zeros_like(params[i]) if g is None else g for g, i in zip(gk, on)]).norm() / total)
    print("gradient shares on to_latent:", {k: f"{v:.3f}" for k, v in shares.items()})
    for k, v in shares.items():
        assert v >= 0.01, f"{k} carries {v:.4f} of the gradient: below the 1 % a wiring error must not hide behind"
    # the gradient of the same call assembled by hand from the public pieces, KL and regularisers as fp32 torch formulas
    out, mean, logvar = m(x, noise=noise)
    reps2 = vae.to_representation(out)
    rgb = vae.render_batch(reps2, ext, intr)["MipGS"]["rgb"]
    from gvfdiffusion_amd.ops.image_loss import image_loss
    img = image_loss(rgb, image, l1_weight=1.0, ssim_weight=LAMBDAS["lambda_ssim"])
    kl = 0.5 * torch.mean(mean.pow(2) + logvar.exp() - logvar - 1)
    vol = torch.prod(torch.cat([r.get_scaling for r in reps2["MipGS"]]), dim=1).mean()
    opa = (torch.cat([r.get_opacity for r in reps2["MipGS"]]) - 1).pow(2).mean()
    hand = img + LAMBDAS["lambda_lpips"] * lp(rgb * 2 - 1, image * 2 - 1) + LAMBDAS["lamda_kl"] * kl + LAMBDAS["lambda_vol"] * vol + \
        LAMBDAS["lambda_opacity"] * opa
    assert abs(float(hand) - float(terms["loss"])) <= 1e-5 * abs(float(hand))
    ref = torch.autograd.grad(hand, params)
    for k, a, b in zip(names, got, ref):
        assert torch.isfinite(a).all() and float(a.abs().max()) > 0, f"{k}: gradient not finite or zero"
        e = R.rel_l2(a, b)
        assert e <= 2.0 ** -8, f"{k}: the gradient of training_losses is {e:.3e} from the hand-assembled call (a wiring error is the size of a term)"


def test_train_step_with_fused_adamw(cuda):
    from gvfdiffusion_amd import training
    from gvfdiffusion_amd.ops.optim import FusedAdamW
    vae, m, x, image, ext, intr, lp, noise = _framework(torch.bfloat16)
    params = [p for p in m.parameters()]
    before = [p.detach().clone() for p in params]
    opt = FusedAdamW(params, lr=1e-3)
    r = training.train_step(params, opt, lambda: training.static_vae_loss(vae, x, image, ext, intr, lpips=lp, noise=noise))
    assert r["found_inf"] == 0 and r["grad_norm"] > 0 and r["grad_norm"] == r["grad_norm"] and r["grad_norm"] != float("inf")
    for (k, p), b in zip(m.named_parameters(), before):
        assert not torch.equal(p.detach(), b), f"{k} did not move"
    r2 = training.train_step(params, opt, lambda: training.static_vae_loss(vae, x, image, ext, intr, lpips=lp))      # drawn noise
    assert r2["found_inf"] == 0 and 0 < r2["grad_norm"] < float("inf") and r2["loss"] == r2["loss"]
