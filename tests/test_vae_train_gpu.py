"""The motion VAE trains on the HIP operators: decode alone and encode_rows -> decode, the shared-query frame sum, several chunks, encode end to
end and a train_step, against float64 autograd of oracle/vae_ref.py.  The unit of every bar is the "yardstick": the same oracle with its
`precision` set to the operand type (fp32 arithmetic, 16-bit roundings where the HIP path rounds), measured against the float64 run; the
kernels get twice its deviation, with the floor of 1e-5 that tests/test_sparse_vae_train_gpu.py uses for a tensor no 16-bit rounding reaches.

Config of tests/vae_train_ref.py (depth 2, dim 192, 3 heads of 64, 40 latents, 64 inputs, T = 3, B = 2, P = 70), loss = sum(logits * W) / n
(+ kl.mean()), fp16 with a loss scale of 1024.  Yardsticks measured on the CPU: bf16 up to 1.2e-2 per tensor, fp16 up to 8.2e-3; to_outputs.bias
1e-7 (a column sum of the loss weights), the only tensor on the floor."""
import pytest
import torch

import vae_train_ref as R

pytestmark = pytest.mark.gpu
DTYPES = [(torch.bfloat16, "bf16"), (torch.float16, "fp16")]
CASES = ["decode", "encode_decode"]
_CACHE = {}


def _cached(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


def _sd():
    return _cached("sd", lambda: {k: v.detach().clone() for k, v in R.model().state_dict().items()})


def _inputs(counts):
    return _cached(("inputs", counts), lambda: R.inputs(counts=counts))


def _ref64(case, counts=(R.P, R.P)):
    return _cached(("ref64", case, counts), lambda: R.oracle_grads(_sd(), R.CFG, _inputs(counts), case))


def _yard(case, name, counts=(R.P, R.P)):
    return _cached(("yard", case, name, counts), lambda: R.oracle_grads(_sd(), R.CFG, _inputs(counts), case, precision=name, dtype=torch.float32))


def _gpu_model(dt, **kw):
    train = {k: kw.pop(k) for k in ("use_checkpoint",) if k in kw}
    m = R.model(**kw)
    return m.cuda().enable_training(dtype=dt, **train)


def _gpu_grads(m, inp, case, est, dt):
    return R.model_grads(m, inp, case, est=est, scale=1024.0 if dt == torch.float16 else 1.0, dev="cuda")


def _hold(tag, got, r64, yard):
    """every gradient <= max(2 x yardstick, 1e-5), the whole gradient <= 2 x the yardstick's whole-gradient figure"""
    assert set(got["grads"]) == set(r64["grads"]), set(got["grads"]) ^ set(r64["grads"])
    log, floor = [], []
    for k in sorted(r64["grads"]):
        g = got["grads"][k]
        e, ey = R.rel_l2(g.cpu(), r64["grads"][k]), R.rel_l2(yard["grads"][k], r64["grads"][k])
        log.append(f"{k} {e:.2e}/{ey:.2e}")
        if 2 * ey < 1e-5:
            floor.append(k)
        assert torch.isfinite(g).all() and e <= max(2 * ey, 1e-5), f"{tag} {k}: rel L2 {e:.3e} > max(2 x {ey:.3e}, 1e-5)"
    assert floor == ["to_outputs.bias"], floor
    keys = sorted(r64["grads"])
    cat = lambda d: torch.cat([d[k].detach().cpu().double().reshape(-1) for k in keys])   # noqa: E731
    e, ey = R.rel_l2(cat(got["grads"]), cat(r64["grads"])), R.rel_l2(cat(yard["grads"]), cat(r64["grads"]))
    el, eyl = R.rel_l2(got["logits"].cpu(), r64["logits"]), R.rel_l2(yard["logits"], r64["logits"])
    print(f"{tag} | kernel/yardstick:", "; ".join(log), f"| whole {e:.2e}/{ey:.2e} | logits {el:.2e}/{eyl:.2e}")
    assert e <= 2 * ey, f"{tag}: whole gradient {e:.3e} > 2 x yardstick {ey:.3e}"
    assert el <= 2 * eyl, f"{tag}: logits {el:.3e} > 2 x yardstick {eyl:.3e}"


@pytest.mark.parametrize("dt,name", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("case", CASES)
def test_every_gradient_against_the_float64_oracle(cuda, case, dt, name):
    """Also: a second run and use_checkpoint on / off give the same bits."""
    inp, r64, yard = _inputs((R.P, R.P)), _ref64(case), _yard(case, name)
    for k, g in r64["grads"].items():
        assert float(g.abs().max()) > 0, f"{k}: zero reference gradient"
    m = _gpu_model(dt, use_checkpoint=False)
    got = _gpu_grads(m, inp, case, r64["est"], dt)
    _hold(f"motion vae {case} {name}", got, r64, yard)
    again = _gpu_grads(m, inp, case, r64["est"], dt)
    ck = _gpu_grads(_gpu_model(dt, use_checkpoint=True), inp, case, r64["est"], dt)
    assert torch.equal(got["logits"], again["logits"]) and torch.equal(got["logits"], ck["logits"])
    for k in got["grads"]:
        assert torch.equal(got["grads"][k], again["grads"][k]), f"{k}: a second run gave other bits"
        assert torch.equal(got["grads"][k], ck["grads"][k]), f"{k}: use_checkpoint gave other bits"


@pytest.mark.parametrize("dt,name", DTYPES, ids=["bf16", "fp16"])
def test_decode_output_against_the_fp32_oracle(cuda, dt, name):
    """the training route's decode within twice the deviation of the operand-type oracle from the fp32 oracle"""
    from oracle import vae_ref
    inp, sd = _inputs((R.P, R.P)), _sd()
    T = R.CFG["num_timesteps"]
    with torch.no_grad():
        ref32 = _cached("dec32", lambda: vae_ref.vae_decode(sd, R.CFG, inp["x"], inp["queries"], T, "fp32"))
        ref16 = vae_ref.vae_decode(sd, R.CFG, inp["x"], inp["queries"], T, name)
    m = _gpu_model(dt)
    y = m.decode(inp["x"].cuda().requires_grad_(), inp["queries"].cuda())
    assert y.grad_fn is not None and y.dtype == torch.float32 and y.shape == ref32.shape
    e, ey = R.rel_l2(y.detach().cpu(), ref32), R.rel_l2(ref16, ref32)
    print(f"motion vae decode, training route [{name}]: rel L2 vs the fp32 oracle {e:.2e}, {name} oracle vs fp32 oracle {ey:.2e}")
    assert e <= 2 * ey


@pytest.mark.parametrize("dt,name", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("case", CASES)
def test_unequal_gaussian_counts_and_ragged_chunks(cuda, case, dt, name):
    """B = 2 with 70 and 55 Gaussians, padded as pad_static_gs pads (the loss weights are 0 on the padding): the shared-query frame sum.
    chunk_size = 32: three chunks, the last of 6 rows, each through torch.utils.checkpoint -- the same bar as the unchunked gradient."""
    counts = (70, 55)
    inp, r64, yard = _inputs(counts), _ref64(case, counts), _yard(case, name, counts)
    one = _gpu_grads(_gpu_model(dt), inp, case, r64["est"], dt)
    _hold(f"motion vae {case} {name} counts {counts}", one, r64, yard)
    three = _gpu_grads(_gpu_model(dt, chunk_size=32), inp, case, r64["est"], dt)
    _hold(f"motion vae {case} {name} counts {counts} chunks of 32", three, r64, yard)
    assert float(one["grads"]["queries"][1, 55:].abs().max()) == 0, "the padding rows carry no loss"


def test_the_switch_leaves_inference_bit_for_bit(cuda):
    inp = _inputs((R.P, R.P))
    x, q = inp["x"].cuda(), inp["queries"].cuda()
    plain = R.model().cuda().set_compute_dtype(torch.bfloat16)
    y0 = plain.decode(x, q)                                               # switch off, grad enabled: no graph, as before
    assert not y0.requires_grad
    m = R.model().cuda().set_compute_dtype(torch.bfloat16).enable_training()
    with torch.no_grad():
        y1 = m.decode(x, q)
    yt = m.decode(x, q)
    m.enable_training(False)
    y2 = m.decode(x, q)
    assert torch.equal(y0, y1) and torch.equal(y0, y2) and not y1.requires_grad and not y2.requires_grad and yt.grad_fn is not None
    e = R.rel_l2(yt.detach(), y0)
    print(f"training vs inference decode [bf16]: rel L2 {e:.2e}")
    assert e < 2e-2


def _encode_inputs():
    g = torch.Generator().manual_seed(2)
    T, N = R.CFG["num_timesteps"], R.CFG["num_inputs"]
    static_pc = torch.rand((2, N, 3), generator=g) - 0.5
    delta_pc = torch.randn((2, T, N, 3), generator=g) * 0.05
    gs = [torch.rand((n, 14), generator=g) - 0.5 for n in (90, 75)]
    return static_pc, delta_pc, gs


def test_encode_end_to_end_on_the_device(cuda):
    """FPS (first Gaussian as the start) and the KNN interpolation under no_grad, then the differentiable rows: kl [B * T], a reproducible
    draw, finite non-zero gradients on every encoder parameter, and a gradient on the static Gaussians through the sampled rows."""
    static_pc, delta_pc, gs = _encode_inputs()
    T, L, Dl = R.CFG["num_timesteps"], R.CFG["num_latents"], R.CFG["latent_dim"]
    noise = torch.randn((2 * T * L, Dl), generator=torch.Generator().manual_seed(5)).cuda()
    m = _gpu_model(torch.bfloat16)
    leaves = [t.cuda().requires_grad_() for t in gs]
    kl, z, post, sampled = m.encode(static_pc.cuda(), delta_pc.cuda(), leaves, random_start=False, noise=noise)
    assert kl.shape == (2 * T,) and z.shape == (2 * T, L, Dl) and sampled.shape == (2, L, 14) and post.mean.shape == z.shape
    kl2, z2, _, _ = m.encode(static_pc.cuda(), delta_pc.cuda(), leaves, random_start=False, noise=noise)
    assert torch.equal(kl, kl2) and torch.equal(z, z2)
    w = torch.randn(z.shape, generator=torch.Generator().manual_seed(6)).cuda()
    enc = {k: p for k, p in m.named_parameters() if k.split(".")[0] in ("input_embedding", "cross_attend_blocks", "mean_fc", "logvar_fc")}
    grads = torch.autograd.grad((z * w).mean() + kl.mean(), list(enc.values()) + leaves)
    for k, g in zip(list(enc) + ["static_gs[0]", "static_gs[1]"], grads):
        assert torch.isfinite(g).all() and float(g.abs().max()) > 0, f"{k}: gradient not finite or zero"
    with torch.no_grad():                                                 # the inference route on the same samples: mean and kl agree
        kl0, z0, post0, sampled0 = m.encode(static_pc.cuda(), delta_pc.cuda(), [t.detach() for t in leaves], random_start=False, sample_posterior=False)
    assert torch.equal(sampled0, sampled.detach())
    assert R.rel_l2(post.mean.detach(), post0.mean) < 2e-2 and R.rel_l2(kl.detach(), kl0) < 2e-2


def test_train_step_with_fused_adamw_through_motion_vae_loss(cuda):
    """One step on a 64 x 64 render of two views a sample: every parameter moves, the loss and the gradient norm are finite."""
    from gvfdiffusion_amd import synthetic, training
    from gvfdiffusion_amd.ops.optim import FusedAdamW
    from gvfdiffusion_amd.renderers import GaussianRenderer
    static_pc, delta_pc, _ = _encode_inputs()
    T = R.CFG["num_timesteps"]
    gms = [synthetic.gaussian_model_from(synthetic.random_gaussians(n, sh_degree=0, seed=3 + i, scale_lo=0.02, scale_hi=0.08), 0, cuda)
           for i, n in enumerate((90, 75))]
    rend = GaussianRenderer({"resolution": 64, "near": synthetic.NEAR, "far": synthetic.FAR, "ssaa": 1, "bg_color": (1, 1, 1)})
    rend.pipe.use_mip_gaussian = True
    rend.pipe.kernel_size = synthetic.KERNEL_2D
    ext = torch.stack([torch.stack([synthetic.orbit_w2c(40.0 * f + 15.0 * b, 10.0) for f in range(2)]) for b in range(2)]).to(cuda)
    K = synthetic.intrinsics().to(cuda)
    g = torch.Generator().manual_seed(8)
    targets = torch.nn.functional.interpolate(torch.rand((4, 3, 8, 8), generator=g), size=(64, 64), mode="bilinear", align_corners=False)
    targets = targets.view(2, 2, 3, 64, 64).to(cuda)
    m = _gpu_model(torch.bfloat16)
    params = list(m.parameters())
    before = [p.detach().clone() for p in params]
    opt = FusedAdamW(params, lr=1e-3)

    def loss_fn():
        return training.motion_vae_loss(m, rend, gms, static_pc.to(cuda), delta_pc.to(cuda), ext, K, targets, frame_of_view=[[0, T - 1], [1, 0]])
    r = training.train_step(params, opt, loss_fn)
    assert r["found_inf"] == 0 and 0 < r["grad_norm"] < float("inf") and r["loss"] == r["loss"] and abs(r["loss"]) < float("inf")
    for (k, p), b in zip(m.named_parameters(), before):
        assert torch.isfinite(p).all() and not torch.equal(p.detach(), b), f"{k} did not move"
    with pytest.raises(RuntimeError):
        m.enable_training(False)
        loss_fn()
