"""Motion-VAE training on the host: the exports and host-side argument checks of include/gvf_vae_train.h, the operators' refusal of CPU
tensors and malformed shapes, the formulas of tests/vae_train_ref.py against float64 autograd of the plain torch expression (the reference's
GEGLU, its embedding through oracle/vae_ref.py::point_embed, its DiagonalGaussianDistribution), the enable_training switch, and the wiring of
the training route through the torch namespace on the CPU in fp32 against float64 autograd of oracle/vae_ref.py.  No GPU needed: nothing
here reaches a launch."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import vae_train_ref as R
from gvfdiffusion_amd import _lib
from gvfdiffusion_amd.ops import vae_train as V

EINVAL, OK = _lib.GVF_EINVAL, _lib.GVF_OK
NAMES = ("gvf_geglu_fwd", "gvf_geglu_bwd", "gvf_vae_embed_train_fwd", "gvf_vae_embed_bwd_workspace_bytes", "gvf_vae_embed_bwd",
         "gvf_posterior_groups_workspace_bytes", "gvf_posterior_groups_fwd", "gvf_posterior_groups_bwd")


def test_header_declarations_are_exported_and_bound():
    from test_capi_symbols import declared_functions
    import gvfdiffusion_amd.ops  # noqa: F401  (the package import registers vae_train's signatures)
    declared = declared_functions()
    l = _lib.lib()
    for n in NAMES:
        assert n in declared and n in _lib.SIGNATURES and hasattr(l, n), n
    from gvfdiffusion_amd import _build
    assert "vae_train.hip" in _build.SOURCES


def test_every_argument_error_is_einval_before_any_launch():
    """fake but aligned addresses: every call below must be refused on the host (a launch would fault)"""
    l = _lib.lib()
    A, ODD4, ODD8 = ctypes.c_void_p(0x10000), ctypes.c_void_p(0x10004), ctypes.c_void_p(0x10008)
    nb = ctypes.c_size_t(0)
    # GEGLU forward: dtype, extents, F not a multiple of 8, leading dimensions (too small, not a multiple of 8), null / misaligned pointers
    assert l.gvf_geglu_fwd(7, A, 32, A, 16, 4, 16, None) == EINVAL
    assert l.gvf_geglu_fwd(0, A, 32, A, 16, -1, 16, None) == EINVAL and l.gvf_geglu_fwd(0, A, 32, A, 16, 4, 0, None) == EINVAL
    assert l.gvf_geglu_fwd(0, A, 24, A, 12, 4, 12, None) == EINVAL
    assert l.gvf_geglu_fwd(0, A, 24, A, 16, 4, 16, None) == EINVAL and l.gvf_geglu_fwd(1, A, 32, A, 8, 4, 16, None) == EINVAL
    assert l.gvf_geglu_fwd(0, A, 36, A, 16, 4, 16, None) == EINVAL and l.gvf_geglu_fwd(0, A, 32, A, 20, 4, 16, None) == EINVAL
    assert l.gvf_geglu_fwd(0, None, 32, A, 16, 4, 16, None) == EINVAL and l.gvf_geglu_fwd(0, A, 32, None, 16, 4, 16, None) == EINVAL
    assert l.gvf_geglu_fwd(0, ODD8, 32, A, 16, 4, 16, None) == EINVAL and l.gvf_geglu_fwd(0, A, 32, ODD8, 16, 4, 16, None) == EINVAL
    assert l.gvf_geglu_fwd(0, None, 32, None, 16, 0, 16, None) == OK                       # empty: no launch
    # GEGLU backward
    assert l.gvf_geglu_bwd(3, A, 32, A, 16, A, 32, 4, 16, None) == EINVAL
    assert l.gvf_geglu_bwd(0, A, 32, A, 16, A, 32, -1, 16, None) == EINVAL and l.gvf_geglu_bwd(0, A, 32, A, 16, A, 32, 4, 20, None) == EINVAL
    assert l.gvf_geglu_bwd(0, A, 24, A, 16, A, 32, 4, 16, None) == EINVAL and l.gvf_geglu_bwd(0, A, 32, A, 8, A, 32, 4, 16, None) == EINVAL
    assert l.gvf_geglu_bwd(0, A, 32, A, 16, A, 24, 4, 16, None) == EINVAL and l.gvf_geglu_bwd(0, A, 32, A, 20, A, 32, 4, 16, None) == EINVAL
    for hole in (1, 3, 5):
        args = [0, A, 32, A, 16, A, 32, 4, 16, None]
        args[hole] = None
        assert l.gvf_geglu_bwd(*args) == EINVAL
        args[hole] = ODD4
        assert l.gvf_geglu_bwd(*args) == EINVAL
    assert l.gvf_geglu_bwd(1, None, 32, None, 16, None, 32, 0, 16, None) == OK
    # embedding: qdim outside 3..16, C not a multiple of 6 / above 768 / 0, negative P, eps, null and misaligned pointers, the workspace
    fwd = [A, 14, A, A, A, A, 10, 192, 1e-5, None]
    for pos, bad in ((1, 2), (1, 17), (7, 190), (7, 774), (7, 0), (6, -1), (8, -1.0)):
        args = list(fwd)
        args[pos] = bad
        assert l.gvf_vae_embed_train_fwd(*args) == EINVAL, (pos, bad)
    for hole in (0, 2, 3, 4, 5):
        args = list(fwd)
        args[hole] = None
        assert l.gvf_vae_embed_train_fwd(*args) == EINVAL
        args[hole] = ctypes.c_void_p(0x10002)
        assert l.gvf_vae_embed_train_fwd(*args) == EINVAL
    assert l.gvf_vae_embed_train_fwd(None, 14, None, None, None, None, 0, 192, 1e-5, None) == OK
    assert l.gvf_vae_embed_bwd_workspace_bytes(10, 2, 192, ctypes.byref(nb)) == EINVAL and l.gvf_vae_embed_bwd_workspace_bytes(10, 14, 100, ctypes.byref(nb)) == EINVAL
    assert l.gvf_vae_embed_bwd_workspace_bytes(-1, 14, 192, ctypes.byref(nb)) == EINVAL and l.gvf_vae_embed_bwd_workspace_bytes(10, 14, 192, None) == EINVAL
    assert l.gvf_vae_embed_bwd_workspace_bytes(4099, 14, 192, ctypes.byref(nb)) == OK and nb.value == 342 * (192 * 14 + 192) * 4     # 12 rows a workgroup
    bwd = [A, 14, A, A, A, A, A, A, A, 4099, 192, 1e-5, A, 1 << 24, None]
    for pos, bad in ((1, 2), (1, 17), (10, 190), (10, 774), (9, -1), (11, -1.0), (13, 64), (12, ODD4)):
        args = list(bwd)
        args[pos] = bad
        assert l.gvf_vae_embed_bwd(*args) == EINVAL, (pos, bad)
    for hole in (0, 2, 3, 4, 5, 6, 7, 12):                                                  # (8 = dr may be null)
        args = list(bwd)
        args[hole] = None
        assert l.gvf_vae_embed_bwd(*args) == EINVAL
    args = list(bwd)
    args[8] = ctypes.c_void_p(0x10002)
    assert l.gvf_vae_embed_bwd(*args) == EINVAL
    assert l.gvf_vae_embed_bwd(None, 14, None, None, None, None, None, None, None, 0, 192, 1e-5, None, 0, None) == OK
    # grouped posterior
    assert l.gvf_posterior_groups_workspace_bytes(3, 0, 16, ctypes.byref(nb)) == EINVAL and l.gvf_posterior_groups_workspace_bytes(3, 40, 0, ctypes.byref(nb)) == EINVAL
    assert l.gvf_posterior_groups_workspace_bytes(-1, 40, 16, ctypes.byref(nb)) == EINVAL and l.gvf_posterior_groups_workspace_bytes(3, 40, 16, None) == EINVAL
    assert l.gvf_posterior_groups_workspace_bytes(3, 513, 8, ctypes.byref(nb)) == OK and nb.value == 3 * 2 * 8
    pf = [A, 16, A, 16, A, A, A, 3, 513, 8, A, 1 << 20, None]
    for pos, bad in ((1, 7), (3, 7), (7, -1), (8, 0), (9, 0), (11, 40), (10, ODD4)):
        args = list(pf)
        args[pos] = bad
        assert l.gvf_posterior_groups_fwd(*args) == EINVAL, (pos, bad)
    for hole in (0, 2, 4, 5, 6, 10):
        args = list(pf)
        args[hole] = None
        assert l.gvf_posterior_groups_fwd(*args) == EINVAL
    assert l.gvf_posterior_groups_fwd(None, 16, None, 16, None, None, None, 0, 513, 8, None, 0, None) == OK
    pb = [A, 16, A, 16, A, A, A, A, 8, A, 8, 3, 513, 8, None]
    for pos, bad in ((1, 7), (3, 7), (8, 7), (10, 7), (11, -1), (12, 0), (13, 0)):
        args = list(pb)
        args[pos] = bad
        assert l.gvf_posterior_groups_bwd(*args) == EINVAL, (pos, bad)
    for hole in (0, 2, 7, 9):
        args = list(pb)
        args[hole] = None
        assert l.gvf_posterior_groups_bwd(*args) == EINVAL
    args = list(pb)
    args[4] = None                                                                          # dz without eps
    assert l.gvf_posterior_groups_bwd(*args) == EINVAL
    assert l.gvf_posterior_groups_bwd(None, 16, None, 16, None, None, None, None, 8, None, 8, 0, 513, 8, None) == OK


def test_operators_refuse_cpu_tensors_and_bad_shapes():
    with pytest.raises(_lib.GvfError):
        V.geglu(torch.zeros((4, 32), dtype=torch.bfloat16))
    with pytest.raises(_lib.GvfError):
        V.embed(torch.zeros((4, 14)), torch.zeros((192, 14)), torch.zeros(192), torch.zeros(32))
    with pytest.raises(_lib.GvfError):
        V.posterior_groups(torch.zeros((8, 16)), torch.zeros((8, 16)), torch.zeros((8, 16)), 2)


# ---- the formulas of the reference file against float64 autograd ------------------------------------------------------------------
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_geglu_formula_equals_float64_autograd(dt):
    """random rows plus gates up to the type's largest finite value (x and da moderate there: the exact result fits a double)"""
    g = torch.Generator().manual_seed(1)
    rows, F_ = 9, 24
    u = (torch.randn((rows, 2 * F_), generator=g) * 3).to(dt).double()
    fmax = torch.finfo(dt).max
    for i, v in enumerate((fmax, -fmax, fmax / 2, -fmax / 2, 40.0, -40.0, 14.0, -14.0, 13.5, -13.5, 6.0, -6.0, 0.0)):
        u[i % rows, F_ + i] = torch.tensor(v).to(dt).double()
    u[0, 0], u[1, 1] = fmax, -fmax                                                          # a huge x beside a huge gate
    da = torch.randn((rows, F_), generator=g).to(dt).double()
    leaf = u.clone().requires_grad_()
    a = leaf[:, :F_] * F.gelu(leaf[:, F_:])
    a.backward(da)
    got = R.geglu(u, da)
    assert torch.isfinite(got["a"]).all() and torch.isfinite(got["du"]).all()
    # element by element (a norm would see the huge cells only); 1e-40: the cut-off term, below 2e-42 of x da
    assert bool(((got["a"] - a.detach()).abs() <= 1e-13 * a.detach().abs()).all())
    assert bool(((got["du"] - leaf.grad).abs() <= 1e-13 * leaf.grad.abs() + 1e-40).all())


@pytest.mark.parametrize("qdim,C", [(6, 192), (14, 192), (14, 768)])
def test_embed_formula_equals_float64_autograd(qdim, C):
    from oracle import vae_ref
    g = torch.Generator().manual_seed(qdim + C)
    P = 37
    r = torch.randn((P, qdim), generator=g, dtype=torch.float64) * 0.4
    W = torch.randn((C, qdim), generator=g, dtype=torch.float64) * 0.3
    b = torch.randn(C, generator=g, dtype=torch.float64) * 0.1
    E = C // 6
    omega = 1.0 / 10000 ** (torch.arange(E, dtype=torch.float64) / (E / 2.0))
    de = torch.randn((P, C), generator=g, dtype=torch.float64)
    rl, Wl, bl = r.clone().requires_grad_(), W.clone().requires_grad_(), b.clone().requires_grad_()
    e = F.layer_norm(F.linear(rl, Wl, bl), (C,), None, None, 1e-5) + F.layer_norm(vae_ref.point_embed(rl[:, :3], omega), (C,), None, None, 1e-5)
    e.backward(de)
    got = R.embed(r, W, b, omega, de)
    assert R.rel_l2(got["e"], e.detach()) < 1e-13
    assert R.rel_l2(got["dW"], Wl.grad) < 1e-12 and R.rel_l2(got["db"], bl.grad) < 1e-12 and R.rel_l2(got["dr"], rl.grad) < 1e-12
    assert float(rl.grad[:, :3].abs().min()) > 0 and float(Wl.grad.abs().min()) > 0


def test_posterior_groups_formula_equals_float64_autograd_with_the_clamp():
    """the reference's DiagonalGaussianDistribution in float64, logvar seeded with values outside and exactly on the clamp's bounds: torch's
    clamp passes the gradient at -30 and 20 and blocks it at -31 and 21"""
    g = torch.Generator().manual_seed(3)
    G, L, Dl = 3, 5, 8
    mean = torch.randn((G * L, Dl), generator=g, dtype=torch.float64)
    logvar = torch.randn((G * L, Dl), generator=g, dtype=torch.float64) * 2
    special = (-31.0, -30.0, 20.0, 21.0)
    for i, v in enumerate(special):
        logvar[i, i] = v
        logvar[L + i, 2] = v
    eps, dz = torch.randn((G * L, Dl), generator=g, dtype=torch.float64) * 1e-3, torch.randn((G * L, Dl), generator=g, dtype=torch.float64)
    dkl = torch.randn(G, generator=g, dtype=torch.float64)
    ml, ll = mean.clone().requires_grad_(), logvar.clone().requires_grad_()
    lv = torch.clamp(ll.view(G, L, Dl), -30.0, 20.0)
    z = ml.view(G, L, Dl) + torch.exp(0.5 * lv) * eps.view(G, L, Dl)
    kl = 0.5 * torch.mean(torch.pow(ml.view(G, L, Dl), 2) + torch.exp(lv) - 1.0 - lv, dim=[1, 2])
    ((z * dz.view(G, L, Dl)).sum() + (kl * dkl).sum()).backward()
    got = R.posterior_groups(mean, logvar, eps, dz, dkl, G)
    assert R.rel_l2(got["z"], z.detach().reshape(G * L, Dl)) < 1e-14 and R.rel_l2(got["kl"], kl.detach()) < 1e-14
    assert R.rel_l2(got["dmean"], ml.grad) < 1e-13 and R.rel_l2(got["dlogvar"], ll.grad) < 1e-13
    for i, v in enumerate(special):
        for cell in ((i, i), (L + i, 2)):
            assert (float(ll.grad[cell]) != 0) == (v in (-30.0, 20.0)) and (float(got["dlogvar"][cell]) != 0) == (v in (-30.0, 20.0))
    only_kl = R.posterior_groups(mean, logvar, eps, None, dkl, G)
    only_z = R.posterior_groups(mean, logvar, eps, dz, None, G)
    assert R.rel_l2(only_kl["dlogvar"] + only_z["dlogvar"], ll.grad) < 1e-13 and R.rel_l2(only_kl["dmean"] + only_z["dmean"], ml.grad) < 1e-13


# ---- the switch -----------------------------------------------------------------------------------------------------------------------
def test_enable_training_is_an_explicit_switch():
    """Off by default; on, only a call with grad enabled takes the training route (seen here by the operator namespace being reached, which
    needs no GPU); off or under no_grad the methods are the inference code, which refuses CPU tensors before anything else."""
    m = R.model()
    assert m._train is None and not m._training_route()
    inp = R.inputs()

    class Reached(Exception):
        pass

    class Probe(R.TorchOps):
        @staticmethod
        def layernorm(x, eps, dtype):
            raise Reached()

    assert m.enable_training(ops=Probe()) is m and m._train.use_checkpoint
    with pytest.raises(Reached):
        m.decode(inp["x"], inp["queries"])
    with pytest.raises(Reached):
        m.decode_latents(inp["x"])
    with torch.no_grad():
        assert not m._training_route()
        with pytest.raises(_lib.GvfError):                 # the inference route: HIP kernels only
            m.decode(inp["x"], inp["queries"])
        with pytest.raises(RuntimeError):
            m.encode_rows(inp["static_pc"], inp["delta_pc"], inp["input_static_gs"], torch.zeros(2, 3, 40, 3))
    m.enable_training(False)
    assert m._train is None
    with pytest.raises(_lib.GvfError):                     # switch off under grad: today's behaviour, no training route
        m.decode(inp["x"], inp["queries"])
    with pytest.raises(ValueError):
        m.enable_training(dtype=torch.float32)
    with pytest.raises(NotImplementedError):
        R.model(decoder_ff=True)


# ---- the wiring through the torch namespace against float64 autograd of the oracle --------------------------------------------------
_REF = {}


def _ref(case):
    if case not in _REF:
        sd = {k: v.detach().clone() for k, v in R.model().state_dict().items()}
        _REF[case] = R.oracle_grads(sd, R.CFG, R.inputs(), case)
    return _REF[case]


@pytest.mark.parametrize("case", ["decode", "encode_decode"])
def test_training_route_through_torch_ops_equals_float64_autograd_of_the_oracle(case):
    """depth 2, dim 192, 3 heads of 64, 40 latents, 64 inputs, T = 3, B = 2, P = 70; loss = sum(logits * W) / n (+ kl.mean()).  Every
    parameter the case uses and `queries` (and the latents for decode alone): fp32 through TorchOps within 1e-5 relative L2 of the float64
    oracle, the same bits with and without use_checkpoint and with three ragged chunks -- and every reference gradient is non-zero, so that
    no bar of tests/test_vae_train_gpu.py is vacuous."""
    ref, inp = _ref(case), R.inputs()
    used = set(ref["grads"])
    params = {k for k, _ in R.model().named_parameters()}
    if case == "encode_decode":
        assert used == params | {"queries"}, "the loss reaches every parameter"
    else:
        assert used == {k for k in params if k.split(".")[0] in ("proj", "layers", "gs_embedding", "decoder_cross_attn", "to_outputs")} | {"queries", "x"}
    for k, g in ref["grads"].items():
        assert float(g.abs().max()) > 0, f"{k}: zero reference gradient"
    runs = {}
    for name, kw in (("plain", dict(use_checkpoint=False)), ("checkpoint", dict(use_checkpoint=True)), ("chunks", dict(use_checkpoint=True, chunk=32))):
        m = R.model(chunk_size=kw.pop("chunk", R.CFG["chunk_size"])).enable_training(ops=R.TorchOps(), **kw)
        runs[name] = R.model_grads(m, inp, case, est=ref["est"])
    got = runs["plain"]
    assert set(got["grads"]) == used
    assert R.rel_l2(got["logits"], ref["logits"]) <= 1e-5 and abs(float(got["loss"]) - float(ref["loss"])) <= 1e-5 * abs(float(ref["loss"]))
    for k in sorted(used):
        e = R.rel_l2(got["grads"][k], ref["grads"][k])
        assert e <= 1e-5, f"{case} {k}: rel L2 {e:.3e}"
        assert torch.equal(got["grads"][k], runs["checkpoint"]["grads"][k]), f"{k}: use_checkpoint gave other bits"
        assert R.rel_l2(runs["chunks"]["grads"][k], ref["grads"][k]) <= 1e-5, f"{k}: three chunks"
    assert torch.equal(got["logits"], runs["checkpoint"]["logits"])


def test_forward_returns_logits_kl_posterior_on_the_training_route(monkeypatch):
    """forward(static_gs, static_pc, delta_pc, noise) = sample -> encode_rows -> decode over the padded Gaussians, with a graph on logits; the
    FPS and the KNN interpolation (HIP kernels) are replaced by the first L Gaussians and the oracle's interpolation here."""
    from gvfdiffusion_amd.model import autoencoder_train as AT
    from oracle import vae_ref
    inp = R.inputs(counts=(70, 55))
    gs = [inp["queries"][0, :70], inp["queries"][1, :55]]
    L = R.CFG["num_latents"]

    def fake_sample(m, static_pc, delta_pc, static_gs_list, random_start):
        sampled = torch.stack([g[:L] for g in static_gs_list])
        return sampled, sampled[..., :3], vae_ref.delta_interp(sampled[..., :3], static_pc, delta_pc + static_pc[:, None])
    monkeypatch.setattr(AT, "_sample", fake_sample)
    m = R.model().enable_training(ops=R.TorchOps())
    out = m(gs, inp["static_pc"], inp["delta_pc"], noise=inp["noise"])
    T = R.CFG["num_timesteps"]
    assert out["logits"].shape == (2, T, 70, 14) and out["logits"].grad_fn is not None and out["kl"].shape == (2 * T,)
    assert out["posterior"].mean.shape == (2 * T, L, 16)
    kl, z, post = m.encode_rows(inp["static_pc"], inp["delta_pc"], inp["input_static_gs"], fake_sample(m, inp["static_pc"], inp["delta_pc"], gs, False)[2],
                                noise=inp["noise"])
    assert torch.equal(kl, out["kl"]) and torch.equal(m.decode(z, inp["queries"]), out["logits"])
