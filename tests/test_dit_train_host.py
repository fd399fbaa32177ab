"""DiT training on the host: the diffusion loss against the reference's own numbers (tests/golden/dit_small_train_golden.npz), the wiring of
model/dit_train.py::forward_train through the torch namespace on the CPU in fp32 against the reference's fp32 gradients, the enable_training
switch, the formulas of tests/dit_train_ref.py against float64 autograd, and the host-side argument checks of include/gvf_dit_train.h.
No GPU needed: nothing here reaches a launch."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dit_train_ref as R
from gvfdiffusion_amd import _lib
from gvfdiffusion_amd.model import dit_train
from gvfdiffusion_amd.model.gaussian_diffusion import GaussianDiffusion, create_gaussian_diffusion, get_named_beta_schedule
from gvfdiffusion_amd.model.resample import UniformSampler, create_named_schedule_sampler


@pytest.fixture(scope="module")
def small():
    return R.load_small("cpu")


# ---- the diffusion loss ---------------------------------------------------------------------------------------------------------------
def test_training_losses_match_the_reference_on_a_fixed_model_output(small):
    _, diffusion, fx = small
    x0, noise, t = torch.from_numpy(fx["x_start"]), torch.from_numpy(fx["noise"]), torch.from_numpy(fx["t"])
    fixed = torch.from_numpy(fx["model_output"])
    seen = {}

    def stub(x, ts, **kw):
        seen["x"], seen["t"], seen["kw"] = x, ts, kw
        return fixed
    terms, aux = diffusion.training_losses(stub, x0, t, model_kwargs={"flag": 1}, noise=noise)
    assert set(aux) == {"x_t", "model_output"} and aux["model_output"] is fixed and seen["kw"] == {"flag": 1}
    # x_t and the target: two products and one add / subtract of fp32 numbers, one rounding each -> 3 half-ulps of the larger magnitude
    eps32 = 2.0 ** -24
    x_t, target = torch.from_numpy(fx["x_t"]), torch.from_numpy(fx["target"])
    bound = 3 * eps32 * (x0.abs() + noise.abs())
    assert bool(((aux["x_t"] - x_t).abs() <= bound).all()) and torch.equal(seen["x"], aux["x_t"])
    assert bool(((diffusion.get_v(x0, noise, t) - target).abs() <= bound).all())
    # rescale_timesteps: the model sees t * 1000 / num_timesteps as a float
    assert seen["t"].dtype == torch.float32 and torch.equal(seen["t"], t.float() * (1000.0 / diffusion.num_timesteps))
    assert terms["mse"].shape == (2,) and terms["loss"].shape == (2,)
    for key, ref in (("mse", fx["mse"]), ("loss", fx["loss_terms"])):
        assert np.allclose(terms[key].numpy(), ref, rtol=1e-6, atol=0), (key, terms[key], ref)
    assert abs(float(terms["loss"].mean()) - float(fx["loss"])) <= 1e-6 * float(fx["loss"])


def test_targets_and_min_snr_weights_by_hand():
    betas = np.array([0.1, 0.2, 0.5])
    abar = np.array([0.9, 0.72, 0.36])                      # cumulative products of 1 - beta
    x0 = torch.tensor([[1.0, -2.0], [0.5, 4.0], [3.0, 0.25]])
    noise = torch.tensor([[0.5, 1.0], [-1.0, 2.0], [0.0, -4.0]])
    t = torch.tensor([0, 2, 1])
    out = torch.tensor([[0.1, 0.2], [0.3, 0.4], [0.5, 0.6]])
    a, s = np.sqrt(abar)[[0, 2, 1]][:, None], np.sqrt(1 - abar)[[0, 2, 1]][:, None]
    want = {"eps": noise.numpy(), "xstart": x0.numpy(), "v": a * noise.numpy() - s * x0.numpy()}
    for ptype in ("eps", "xstart", "v"):
        for min_snr in (False, True):
            d = GaussianDiffusion(betas, predict_type=ptype, min_snr=min_snr)
            terms, aux = d.training_losses(lambda x, ts: out, x0, t, noise=noise)
            assert np.allclose(aux["x_t"].numpy(), a * x0.numpy() + s * noise.numpy(), rtol=1e-6)
            mse = ((want[ptype] - out.numpy()) ** 2).mean(axis=1)
            assert np.allclose(terms["mse"].numpy(), mse, rtol=1e-6)
            w = np.minimum((abar / (1 - abar))[[0, 2, 1]], 5.0) if min_snr else np.ones(3)      # SNR = abar / (1 - abar) = 9, 0.5625, 2.571
            assert np.allclose(terms["loss"].numpy(), mse * w, rtol=1e-6)
    assert np.isclose(np.minimum(abar / (1 - abar), 5.0)[0], 5.0)                                 # the clamp is exercised
    # SNR 0 (abar = 0) takes weight 1
    d = GaussianDiffusion(np.array([0.5, 1.0]), predict_type="eps", min_snr=True)
    terms, _ = d.training_losses(lambda x, ts: torch.zeros(1, 2), torch.ones(1, 2), torch.tensor([1]), noise=torch.ones(1, 2))
    assert np.allclose(terms["loss"].numpy(), terms["mse"].numpy())
    # without rescale_timesteps the model sees the integer steps
    got = {}
    GaussianDiffusion(betas).training_losses(lambda x, ts: (got.setdefault("t", ts), out)[1], x0, t, noise=noise)
    assert got["t"] is t


def test_unsupported_diffusion_options_raise():
    for kw in (dict(learn_sigma=True), dict(use_kl=True)):
        d = create_gaussian_diffusion(steps=100, **kw)
        with pytest.raises(NotImplementedError):
            d.training_losses(lambda x, ts: x, torch.zeros(1, 2), torch.tensor([3]))
    with pytest.raises(NotImplementedError):
        create_gaussian_diffusion(steps=100, timestep_respacing="5")
    d = create_gaussian_diffusion(steps=100, min_snr=True, predict_type="v")
    assert d.min_snr and d.predict_type == "v" and np.array_equal(d.betas.shape, (100,))
    assert np.allclose(np.cumprod(1 - d.betas), np.cumprod(1 - get_named_beta_schedule("linear", 100)))


def test_uniform_sampler():
    s = create_named_schedule_sampler("uniform", GaussianDiffusion(np.full(50, 0.01)))
    assert isinstance(s, UniformSampler)
    t, w = s.sample(4096, torch.device("cpu"))
    assert t.dtype == torch.int64 and t.shape == (4096,) and int(t.min()) >= 0 and int(t.max()) < 50 and len(set(t.tolist())) > 25
    assert w.dtype == torch.float32 and bool((w == 1).all())
    with pytest.raises(NotImplementedError):
        create_named_schedule_sampler("loss-second-moment", GaussianDiffusion(np.full(5, 0.01)))


# ---- the wiring of forward_train, CPU fp32 through the torch namespace -----------------------------------------------------------------
def _grads(model, diffusion, fx, checkpoint=False):
    for blk in model.blocks:
        blk.use_checkpoint = checkpoint
    model.zero_grad(set_to_none=True)
    ops = R.TorchOps()
    fwd = lambda x, ts, **kw: dit_train.forward_train(model, x, ts, ops=ops, dtype=torch.float32, **kw)
    terms, _ = diffusion.training_losses(fwd, torch.from_numpy(fx["x_start"]), torch.from_numpy(fx["t"]), model_kwargs=fx["cond"],
                                         noise=torch.from_numpy(fx["noise"]))
    loss = terms["loss"].mean()
    loss.backward()
    for blk in model.blocks:
        blk.use_checkpoint = False
    return float(loss.detach()), {n: p.grad.clone() for n, p in model.named_parameters()}


def test_forward_train_gradients_match_the_reference_fp32(small):
    """Every parameter's gradient within 1e-5 relative L2 of the reference's fp32 gradient (two independent fp32 compositions agree to
    1.5e-7 per tensor here; a wiring error is percent-sized), none skipped; with use_checkpoint the gradients are equal."""
    model, diffusion, fx = small
    loss, grads = _grads(model, diffusion, fx)
    assert abs(loss - float(fx["loss"])) <= 1e-6 * float(fx["loss"])
    names = [n for n, _ in model.named_parameters()]
    assert sum(p.numel() for p in model.parameters()) == int(fx["n_params"]) == 309328
    worst = 0.0
    for n in names:
        assert "grad." + n in fx, f"the fixture has no gradient for {n}"
        ref = torch.from_numpy(fx["grad." + n])
        assert float(ref.abs().max()) > 0
        e = R.rel_l2(grads[n], ref)
        worst = max(worst, e)
        assert e <= 1e-5, (n, e)
    print(f"forward_train fp32 vs reference fp32 gradients: worst per-tensor rel L2 {worst:.2e} over {len(names)} tensors")
    assert {k[5:] for k in fx if k.startswith("grad.")} == set(names)
    loss_c, grads_c = _grads(model, diffusion, fx, checkpoint=True)
    assert loss_c == loss
    for n in names:
        assert torch.equal(grads_c[n], grads[n]), n


def test_enable_training_is_off_by_default_and_never_reached(small, monkeypatch):
    model, _, fx = small
    assert model.train_forward is False and model.training
    hits = []
    monkeypatch.setattr(dit_train, "forward_train", lambda *a, **k: hits.append(1) or "train")
    monkeypatch.setattr(type(model), "_forward", lambda self, *a, **k: "inference")
    args = (torch.zeros(1, 1, 4, 16), torch.zeros(1), torch.zeros(1, 1, 3, 32), torch.zeros(1, 5, 14), torch.zeros(1, 4, 3))
    assert model(*args) == "inference" and not hits                       # grad enabled, parameters require grad, training mode: still inference
    try:
        assert model.enable_training() is model
        assert model(*args) == "train" and hits == [1]
        with torch.no_grad():
            assert model(*args) == "inference"
        model.enable_graph(True)
        with pytest.raises(RuntimeError, match="enable_graph"):
            model(*args)
    finally:
        model.enable_graph(False)
        model.enable_training(False)
    assert model(*args) == "inference" and hits == [1]


def test_hip_namespace_refuses_cpu_tensors_and_fp32_operands(small):
    model, _, fx = small
    x = torch.from_numpy(fx["x_t"])
    with pytest.raises(ValueError):
        dit_train.forward_train(model, x, torch.from_numpy(fx["t"]), dtype=torch.float32, **fx["cond"])
    with pytest.raises(_lib.GvfError):
        dit_train.forward_train(model, x, torch.from_numpy(fx["t"]), dtype=torch.bfloat16, **fx["cond"])
    from gvfdiffusion_amd import training
    with pytest.raises(ValueError, match="mem_ratio"):
        training.diffusion_loss(None, None, x, {"mem_ratio": 1.0})


# ---- the reference formulas against float64 autograd -----------------------------------------------------------------------------------
def test_reference_formulas_against_autograd():
    g = torch.Generator().manual_seed(3)
    rows, C, rpg = 11, 20, 4
    G = (rows + rpg - 1) // rpg
    f64 = torch.float64
    x, dy, dres = (torch.randn((rows, C), generator=g, dtype=f64) for _ in range(3))
    w, b = torch.randn(C, generator=g, dtype=f64), torch.randn(C, generator=g, dtype=f64)
    sh, sc = torch.randn((G, C), generator=g, dtype=f64), torch.randn((G, C), generator=g, dtype=f64)
    gi = torch.arange(rows) // rpg
    leaves = [t.requires_grad_() for t in (x, w, b, sh, sc)]
    y = (F.layer_norm(x, (C,), w, b, 1e-6) * (1 + sc[gi]) + sh[gi])
    gr = torch.autograd.grad((y * dy).sum() + (x * dres).sum(), leaves)
    out = R.ln_mod(x.detach(), dy, dres, w.detach(), b.detach(), sh.detach(), sc.detach(), rpg)
    for got, want in zip((out["dx"], out["dw"], out["db"], out["dshift"], out["dscale"]), gr):
        assert R.rel_l2(got, want) < 1e-12
    assert R.rel_l2(out["y"], y.detach()) < 1e-14
    # gate
    h, dout = torch.randn((rows, C), generator=g, dtype=f64).requires_grad_(), torch.randn((rows, C), generator=g, dtype=f64)
    gt = torch.randn((G, C), generator=g, dtype=f64).requires_grad_()
    o = x.detach() + gt[gi] * h
    gh, gg = torch.autograd.grad((o * dout).sum(), (h, gt))
    out = R.gate(x.detach(), h.detach(), dout, gt.detach(), rpg)
    assert R.rel_l2(out["out"], o.detach()) < 1e-14 and R.rel_l2(out["dh"], gh) < 1e-14 and R.rel_l2(out["dgate"], gg) < 1e-13
    # RMSNorm, with an all-zero row: dx = u / 1e-12, what torch gives
    H, d = 3, 32
    xq = torch.randn((rows, H, d), generator=g, dtype=f64)
    xq[4, 1] = 0
    xq.requires_grad_()
    gm = torch.randn((H, d), generator=g, dtype=f64).requires_grad_()
    dyq = torch.randn((rows, H, d), generator=g, dtype=f64)
    yq = F.normalize(xq, dim=-1) * gm * d ** 0.5
    gx, ggm = torch.autograd.grad((yq * dyq).sum(), (xq, gm))
    out = R.rms(xq.detach(), dyq, gm.detach())
    assert R.rel_l2(out["y"], yq.detach()) < 1e-14 and R.rel_l2(out["dx"], gx) < 1e-12 and R.rel_l2(out["dgamma"], ggm) < 1e-12
    assert float(out["dx"][4, 1].abs().max()) > 1e9
    # the yardstick is the same computation in fp32
    y32 = R.rms(xq.detach().float(), dyq.float(), gm.detach().float(), dtype=torch.float32, lp=torch.bfloat16)
    assert R.rel_l2(y32["dgamma"], ggm) < 1e-5 and R.rel_l2(y32["y"], yq.detach()) < 4e-3


# ---- the C entry points refuse bad arguments on the host -------------------------------------------------------------------------------
def _vp(x):
    return None if x is None else ctypes.c_void_p(x)


def _query(name, *dims):
    out = ctypes.c_size_t(0)
    return getattr(_lib.lib(), name)(*dims, ctypes.byref(out)), int(out.value)


def _ln_bwd(**over):
    """gvf_ln_mod_bwd with plausible host-side values (the pointers are never dereferenced: every case here is refused first)."""
    a = dict(dtype=0, x=0x10000, dy=0x20000, dres=0x30000, dx=0x40000, rows=37, C=512, ln_w=0x50000, ln_b=0x60000, scale=0x70000, mod_ld=3072,
             rpg=10, dshift=0x80000, dscale=0x90000, dw=0xa0000, db=0xb0000, ws=0xc0000, ws_bytes=None)
    a.update(over)
    if a["ws_bytes"] is None:
        a["ws_bytes"] = _query("gvf_ln_mod_bwd_workspace_bytes", 37, 512, 10)[1]
    return _lib.lib().gvf_ln_mod_bwd(a["dtype"], _vp(a["x"]), _vp(a["dy"]), _vp(a["dres"]), _vp(a["dx"]), a["rows"], a["C"], 1e-6, _vp(a["ln_w"]),
                                     _vp(a["ln_b"]), _vp(a["scale"]), a["mod_ld"], a["rpg"], _vp(a["dshift"]), _vp(a["dscale"]), _vp(a["dw"]),
                                     _vp(a["db"]), _vp(a["ws"]), a["ws_bytes"], None)


@pytest.mark.parametrize("over", [dict(x=None), dict(dy=None), dict(dx=None), dict(ws=None), dict(dtype=2), dict(dtype=-1), dict(rows=-1), dict(C=0),
                                  dict(ln_b=None), dict(ln_w=None), dict(dw=None), dict(db=None), dict(dshift=None), dict(dscale=None),
                                  dict(scale=None), dict(ln_w=None, ln_b=None), dict(rpg=0), dict(mod_ld=511), dict(mod_ld=514),
                                  dict(x=0x10004), dict(dx=0x40008), dict(dres=0x30004), dict(dy=0x20002), dict(ln_w=0x50004), dict(scale=0x70008),
                                  dict(ws=0xc0004), dict(ws_bytes=0), dict(ws_bytes=1000)])
def test_ln_mod_bwd_refuses_bad_arguments_on_the_host(over):
    assert _ln_bwd(**over) == _lib.GVF_EINVAL


def test_workspace_queries_and_empty_calls():
    rc, nb = _query("gvf_ln_mod_bwd_workspace_bytes", 37, 512, 10)
    assert rc == _lib.GVF_OK and nb == (2 * (3 + 4) + 2 * 3) * 512 * 4          # 3 workgroups of 16 rows, 4 groups of 10
    assert _query("gvf_ln_mod_bwd_workspace_bytes", 12288, 512, 12288)[1] == (2 * 769 + 2 * 768) * 512 * 4
    assert _query("gvf_gate_residual_bwd_workspace_bytes", 37, 100, 10) == (_lib.GVF_OK, (3 + 4) * 100 * 4)
    assert _query("gvf_rmsnorm_heads_bwd_workspace_bytes", 130, 16, 32) == (_lib.GVF_OK, 9 * 512 * 4)
    for name, bad in (("gvf_ln_mod_bwd_workspace_bytes", (-1, 512, 10)), ("gvf_ln_mod_bwd_workspace_bytes", (4, 0, 10)),
                      ("gvf_gate_residual_bwd_workspace_bytes", (4, 8, -1)), ("gvf_rmsnorm_heads_bwd_workspace_bytes", (4, 2, 48)),
                      ("gvf_rmsnorm_heads_bwd_workspace_bytes", (4, 0, 32)), ("gvf_rmsnorm_heads_bwd_workspace_bytes", (4, 65, 32))):
        assert _query(name, *bad)[0] == _lib.GVF_EINVAL
        assert getattr(_lib.lib(), name)(4, 32, 32, None) == _lib.GVF_EINVAL
    l = _lib.lib()
    # rows == 0: GVF_OK without a launch, whatever the pointers
    assert _ln_bwd(rows=0, x=None, ws=None) == _lib.GVF_OK
    assert l.gvf_gate_residual_fwd(0, None, None, None, 0, 0, None, 0, 512, None) == _lib.GVF_OK
    assert l.gvf_gate_residual_bwd(1, None, None, None, 0, 0, None, None, 0, 512, None, 0, None) == _lib.GVF_OK
    assert l.gvf_rmsnorm_heads_fwd(0, None, 0, None, None, 0, 0, 16, 32, None) == _lib.GVF_OK
    assert l.gvf_rmsnorm_heads_bwd(0, None, 0, None, 0, None, None, 0, None, 0, 16, 32, None, 0, None) == _lib.GVF_OK


def test_gate_and_rmsnorm_refuse_bad_arguments_on_the_host():
    l = _lib.lib()
    E = _lib.GVF_EINVAL
    fwd = lambda dtype=0, x=0x10000, h=0x20000, gate=0x30000, ld=1536, rpg=10, out=0x40000, rows=37, C=512: \
        l.gvf_gate_residual_fwd(dtype, _vp(x), _vp(h), _vp(gate), ld, rpg, _vp(out), rows, C, None)
    for kw in (dict(dtype=3), dict(x=None), dict(h=None), dict(out=None), dict(rpg=0), dict(ld=100), dict(ld=1538), dict(x=0x10008), dict(h=0x20004),
               dict(gate=0x30004), dict(out=0x40004), dict(rows=-2), dict(C=0)):
        assert fwd(**kw) == E, kw
    nb = _query("gvf_gate_residual_bwd_workspace_bytes", 37, 512, 10)[1]
    bwd = lambda dtype=0, dout=0x10000, h=0x20000, gate=0x30000, ld=1536, rpg=10, dh=0x40000, dgate=0x50000, rows=37, C=512, ws=0x60000, nb=nb: \
        l.gvf_gate_residual_bwd(dtype, _vp(dout), _vp(h), _vp(gate), ld, rpg, _vp(dh), _vp(dgate), rows, C, _vp(ws), nb, None)
    for kw in (dict(dtype=2), dict(dout=None), dict(dh=None), dict(h=None), dict(dgate=None), dict(gate=None), dict(ws=None), dict(nb=nb - 1), dict(rpg=0),
               dict(ld=8), dict(dout=0x10004), dict(dh=0x40002), dict(ws=0x60008), dict(gate=0x30008)):
        assert bwd(**kw) == E, kw
    rf = lambda dtype=0, x=0x10000, ldx=1536, gamma=0x20000, y=0x30000, ldy=512, rows=37, H=16, d=32: \
        l.gvf_rmsnorm_heads_fwd(dtype, _vp(x), ldx, _vp(gamma), _vp(y), ldy, rows, H, d, None)
    for kw in (dict(dtype=5), dict(x=None), dict(gamma=None), dict(y=None), dict(d=16), dict(d=128), dict(H=0), dict(H=65), dict(ldx=500), dict(ldx=1540),
               dict(ldy=516), dict(x=0x10008), dict(y=0x30004), dict(gamma=0x20004), dict(rows=-1)):
        assert rf(**kw) == E, kw
    nb = _query("gvf_rmsnorm_heads_bwd_workspace_bytes", 37, 16, 32)[1]
    rb = lambda dtype=1, x=0x10000, ldx=1536, dy=0x20000, lddy=512, gamma=0x30000, dx=0x40000, lddx=512, dgamma=0x50000, rows=37, H=16, d=32, ws=0x60000, nb=nb: \
        l.gvf_rmsnorm_heads_bwd(dtype, _vp(x), ldx, _vp(dy), lddy, _vp(gamma), _vp(dx), lddx, _vp(dgamma), rows, H, d, _vp(ws), nb, None)
    for kw in (dict(dtype=2), dict(x=None), dict(dy=None), dict(gamma=None), dict(dx=None), dict(dgamma=None), dict(ws=None), dict(nb=nb - 4), dict(d=48),
               dict(lddy=508), dict(lddx=520 + 4), dict(dy=0x20008), dict(dx=0x40002), dict(ws=0x60004)):
        assert rb(**kw) == E, kw
