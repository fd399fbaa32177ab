"""The DiT trains with its block projections on this library's own GEMMs: the model-level tests of tests/test_dit_train_gpu.py with
enable_training(linear="hip") / forward_train(linear="hip"), on the same fixtures and against the same yardsticks -- every parameter's gradient
within twice the relative L2 by which the reference's torch.autocast run of that type deviates from its fp32 gradient for that tensor, the
whole gradient within twice the reference's whole-gradient figure, the loss within the reference's own loss deviation; equal bits run to run
and under use_checkpoint; the C 256 model within twice the error of the torch namespace rounded at the same points.  The measured ratios are
printed (python -m pytest -s) and recorded in profiles/r16_linear_grad.txt."""
import copy

import pytest
import torch

import dit_train_ref as R

pytestmark = pytest.mark.gpu
DTYPES = [(torch.bfloat16, "bf16", 1.0), (torch.float16, "fp16", 1024.0)]


@pytest.fixture(scope="module")
def small(cuda):
    model, diffusion, fx = R.load_small(cuda)
    fx["dev"] = {k: torch.from_numpy(fx[k]).to(cuda) for k in ("x_start", "t", "noise")}
    return model, diffusion, fx


_CACHE = {}


def _run(small, dt, scale, checkpoint=False, fresh=False):
    """(loss, {name: unscaled fp32 gradient}) of one training forward + backward with linear="hip"; computed once per (type, checkpoint)."""
    key = (dt, checkpoint)
    if key in _CACHE and not fresh:
        return _CACHE[key]
    model, diffusion, fx = small
    model.enable_training(linear="hip").set_compute_dtype(dt)
    for blk in model.blocks:
        blk.use_checkpoint = checkpoint
    try:
        model.zero_grad(set_to_none=True)
        d = fx["dev"]
        terms, aux = diffusion.training_losses(model, d["x_start"], d["t"], model_kwargs=fx["cond"], noise=d["noise"])
        assert aux["model_output"].grad_fn is not None and aux["model_output"].dtype == torch.float32
        loss = terms["loss"].mean()
        (loss * scale).backward()
        out = (float(loss.detach()), {n: (p.grad.detach() / scale).cpu() for n, p in model.named_parameters()})
        assert all(p.grad.dtype == torch.float32 for p in model.parameters())
    finally:
        model.enable_training(False).set_compute_dtype(None)
        for blk in model.blocks:
            blk.use_checkpoint = False
        model.zero_grad(set_to_none=True)
    if not fresh:
        _CACHE[key] = out
    return out


@pytest.mark.parametrize("dt,name,scale", DTYPES, ids=["bf16", "fp16"])
def test_gradients_within_twice_the_references_own_autocast_deviation(small, dt, name, scale):
    model, _, fx = small
    loss, grads = _run(small, dt, scale)
    names = [n for n, _ in model.named_parameters()]
    assert {k[5:] for k in fx if k.startswith("grad.")} == set(names)
    lines, bad = [], []
    for n in names:
        e, bar = R.rel_l2(grads[n], torch.from_numpy(fx["grad." + n])), float(fx[f"rel_{name}.{n}"])
        lines.append(f"  {n}: {e:.3e} / {bar:.3e} = {e / bar:.2f}")
        if not e <= 2 * bar:
            bad.append(lines[-1])
    flat = torch.cat([grads[n].reshape(-1) for n in names])
    ref = torch.cat([torch.from_numpy(fx["grad." + n]).reshape(-1) for n in names])
    tot, tot_bar = R.rel_l2(flat, ref), float(fx[f"rel_{name}_total"])
    dl, dl_bar = abs(loss - float(fx["loss"])) / float(fx["loss"]), float(fx[f"loss_rel_{name}"])
    print(f"dit_small training, linear=hip, {name} (loss scale {scale:g}): rel L2 of the gradient against the reference's fp32 gradient / the reference's own autocast figure")
    print("\n".join(lines))
    print(f"  whole gradient: {tot:.3e} / {tot_bar:.3e} = {tot / tot_bar:.2f};  loss {loss:.7f} vs {float(fx['loss']):.7f}: {dl:.3e} / {dl_bar:.3e}")
    assert not bad, "gradients beyond twice the reference's own autocast deviation:\n" + "\n".join(bad)
    assert tot <= 2 * tot_bar
    assert dl <= dl_bar, f"loss deviates {dl:.3e} from the fp32 loss, the reference's own {name} run {dl_bar:.3e}"


@pytest.mark.parametrize("dt,name,scale", DTYPES, ids=["bf16", "fp16"])
def test_two_runs_and_checkpointing_give_equal_bits(small, dt, name, scale):
    loss, grads = _run(small, dt, scale)
    loss2, grads2 = _run(small, dt, scale, fresh=True)
    loss3, grads3 = _run(small, dt, scale, checkpoint=True)
    assert loss2 == loss and loss3 == loss
    for n in grads:
        assert torch.equal(grads2[n], grads[n]), f"a second run gave other bits in {n}"
        assert torch.equal(grads3[n], grads[n]), f"use_checkpoint gave other bits in {n}"


def test_each_weight_is_cast_once_per_step_also_under_checkpointing(small, monkeypatch):
    from gvfdiffusion_amd.ops import linear_grad
    model, _, _ = small
    n = {"cast": 0}
    real = linear_grad.cast_transpose
    monkeypatch.setattr(linear_grad, "cast_transpose", lambda *a, **k: (n.__setitem__("cast", n["cast"] + 1), real(*a, **k))[1])
    per_block = 10 + (0 if model.blocks[0].no_temporal_attn else 2)
    for checkpoint in (False, True):
        n["cast"] = 0
        _run(small, torch.bfloat16, 1.0, checkpoint=checkpoint, fresh=True)
        assert n["cast"] == per_block * len(model.blocks), (checkpoint, n["cast"])


def test_train_step_with_fused_adamw(small):
    from gvfdiffusion_amd.ops.optim import FusedAdamW
    from gvfdiffusion_amd.training import diffusion_loss, train_step
    model, diffusion, fx = small
    net = copy.deepcopy(model).enable_training(linear="hip").set_compute_dtype(torch.bfloat16)
    before = {n: p.detach().clone() for n, p in net.named_parameters()}
    params = list(net.parameters())
    opt = FusedAdamW(params, lr=1e-3, weight_decay=0.0)
    d = fx["dev"]
    info = train_step(params, opt, lambda: diffusion_loss(diffusion, net, d["x_start"], fx["cond"], t=d["t"], noise=d["noise"]), max_grad_norm=1.0)
    assert info["found_inf"] == 0 and info["grad_norm"] > 0 and info["grad_norm"] == info["grad_norm"] and info["grad_norm"] < float("inf")
    assert abs(info["loss"] - float(fx["loss"])) < 1e-3
    for n, p in net.named_parameters():
        assert not torch.equal(p.detach(), before[n]), f"{n} did not move"
        assert bool(torch.isfinite(p).all())
    info2 = train_step(params, opt, lambda: diffusion_loss(diffusion, net, d["x_start"], fx["cond"]), max_grad_norm=1.0)      # sampled t and noise
    assert info2["found_inf"] == 0 and info2["loss"] == info2["loss"]


@pytest.mark.parametrize("dt,name,scale", DTYPES, ids=["bf16", "fp16"])
def test_wide_model_takes_the_vector_kernels(cuda, dt, name, scale):
    """C 256 (8 heads of 32, one block, T 2, N 64, random weights) with linear="hip".  Reference: the same forward through the torch namespace in
    float64 on the same device; yardstick: TorchOps(attention="kernel_points") in the operand type.  Every gradient within twice the
    yardstick's own error."""
    from gvfdiffusion_amd.model.dit import DiT
    from gvfdiffusion_amd.model import dit_train
    torch.manual_seed(5)
    cfg = dict(resolution=64, in_channels=16, model_channels=256, static_cond_channels=14, image_cond_channels=32, out_channels=16, num_blocks=1,
               num_heads=8, mlp_ratio=4, pe_mode="ape", qk_rms_norm=True, qk_rms_norm_cross=True, use_fp16=False, no_temporal_attn=False)
    net = DiT(**cfg)
    g = torch.Generator().manual_seed(6)
    with torch.no_grad():
        for p in net.parameters():                               # the zero-initialised adaLN / head and the unit gains: re-drawn
            if float(p.abs().max()) == 0:
                p.copy_(torch.randn(p.shape, generator=g) * 0.02)
            elif bool((p == 1).all()):
                p.copy_(1 + 0.1 * torch.randn(p.shape, generator=g))
    net = net.to(cuda)
    B, T, N = 2, 2, 64
    x = torch.randn((B, T, N, 16), generator=g).to(cuda)
    t = torch.tensor([900.0, 120.0], device=cuda)
    cond = dict(cond_images=torch.randn((B, T, 37, 32), generator=g).to(cuda), static_latent=torch.randn((B, 50, 14), generator=g).to(cuda),
                deformation_position_xyz=(torch.rand((B, N, 3), generator=g) - 0.5).to(cuda))
    target = torch.randn((B, T, N, 16), generator=g).to(cuda)

    def grads_of(model, ops, dtype, s, linear="torch"):
        model.zero_grad(set_to_none=True)
        y = dit_train.forward_train(model, x.to(next(model.parameters()).dtype), t, ops=ops, dtype=dtype, linear=linear,
                                    **{k: v.to(next(model.parameters()).dtype) for k, v in cond.items()})
        loss = ((y.float() - target) ** 2).mean()
        (loss * s).backward()
        return float(loss.detach()), {n: (p.grad.detach().double() / s).cpu() for n, p in model.named_parameters()}

    ref_net = copy.deepcopy(net).double()
    l64, g64 = grads_of(ref_net, R.TorchOps(), torch.float64, 1.0)
    ly, gy = grads_of(net, R.TorchOps(attention="kernel_points"), dt, scale)
    lk, gk = grads_of(net, None, dt, scale, linear="hip")
    lines, bad = [], []
    for n in g64:
        e, ey = R.rel_l2(gk[n], g64[n]), R.rel_l2(gy[n], g64[n])
        lines.append(f"  {n}: {e:.3e} / {ey:.3e} = {e / ey:.2f}")
        if not e <= 2 * ey:
            bad.append(lines[-1])
    print(f"C 256 model, linear=hip, {name}: rel L2 against float64, HIP operators / torch namespace at the same rounding points; loss {lk:.6f} / {ly:.6f} / {l64:.6f}")
    print("\n".join(lines))
    assert not bad, "gradients beyond twice the yardstick's own error:\n" + "\n".join(bad)
