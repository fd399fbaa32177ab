"""Static-VAE training on the host: the exports and host-side argument checks of include/gvf_sparse_train.h, the operators' refusal of CPU
tensors, the enable_training switch, the errors of SparseVAE.training_losses, the formulas of tests/sparse_train_ref.py against float64
autograd, and the wiring of the training forward through the torch namespace on the CPU in fp32 against float64 autograd of
oracle/sparse_vae_ref.py at the golden config.  No GPU needed: nothing here reaches a launch."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import sparse_train_ref as R
from gvfdiffusion_amd import _lib, sparse as sp
from gvfdiffusion_amd.model.sparse_voxel_diffusion import SparseTransformerVAE, SparseVAE
from gvfdiffusion_amd.ops import sparse_train as S

EINVAL = _lib.GVF_EINVAL
NAMES = ("gvf_gelu_tanh_fwd", "gvf_gelu_tanh_bwd", "gvf_gather_rows", "gvf_posterior_workspace_bytes", "gvf_posterior_fwd", "gvf_posterior_bwd",
         "gvf_gaussian_reg_workspace_bytes", "gvf_gaussian_reg_fwd", "gvf_gaussian_reg_bwd", "gvf_colsum_f32_workspace_bytes", "gvf_colsum_f32")


def test_header_declarations_are_exported_and_bound():
    from test_capi_symbols import declared_functions
    declared = declared_functions()
    l = _lib.lib()
    for n in NAMES:
        assert n in declared and n in _lib.SIGNATURES and hasattr(l, n), n


def test_every_argument_error_is_einval_before_any_launch():
    """fake but aligned addresses: every call below must be refused on the host (a launch would fault)"""
    l = _lib.lib()
    A, ODD = ctypes.c_void_p(0x10000), ctypes.c_void_p(0x10004)
    nb = ctypes.c_size_t(0)
    # GELU: dtype, negative n, null pointers, a pointer that is not even 2-byte aligned
    assert l.gvf_gelu_tanh_fwd(7, A, A, 8, None) == EINVAL
    assert l.gvf_gelu_tanh_fwd(0, A, A, -1, None) == EINVAL
    assert l.gvf_gelu_tanh_fwd(0, None, A, 8, None) == EINVAL and l.gvf_gelu_tanh_fwd(1, A, None, 8, None) == EINVAL
    assert l.gvf_gelu_tanh_fwd(0, ctypes.c_void_p(0x10001), A, 8, None) == EINVAL
    assert l.gvf_gelu_tanh_bwd(0, A, None, A, 8, None) == EINVAL and l.gvf_gelu_tanh_bwd(3, A, A, A, 8, None) == EINVAL
    assert l.gvf_gelu_tanh_fwd(0, None, None, 0, None) == _lib.GVF_OK                  # empty: no launch
    # gather: width not a multiple of 16, stride below the width or unaligned, null / misaligned pointers
    assert l.gvf_gather_rows(A, 32, A, A, 4, 24, None) == EINVAL
    assert l.gvf_gather_rows(A, 16, A, A, 4, 32, None) == EINVAL
    assert l.gvf_gather_rows(A, 40, A, A, 4, 32, None) == EINVAL
    assert l.gvf_gather_rows(A, 32, A, A, -1, 32, None) == EINVAL
    assert l.gvf_gather_rows(None, 32, A, A, 4, 32, None) == EINVAL and l.gvf_gather_rows(A, 32, None, A, 4, 32, None) == EINVAL
    assert l.gvf_gather_rows(A, 32, A, None, 4, 32, None) == EINVAL and l.gvf_gather_rows(ODD, 32, A, A, 4, 32, None) == EINVAL
    assert l.gvf_gather_rows(A, 32, ODD, A, 4, 32, None) == EINVAL
    assert l.gvf_gather_rows(None, 32, None, None, 0, 32, None) == _lib.GVF_OK
    # posterior
    assert l.gvf_posterior_workspace_bytes(10, 0, ctypes.byref(nb)) == EINVAL and l.gvf_posterior_workspace_bytes(-1, 8, ctypes.byref(nb)) == EINVAL
    assert l.gvf_posterior_workspace_bytes(10, 8, None) == EINVAL
    assert l.gvf_posterior_workspace_bytes(4099, 8, ctypes.byref(nb)) == _lib.GVF_OK and nb.value == 8 * ((4099 * 8 + 4095) // 4096)
    assert l.gvf_posterior_fwd(A, 15, A, A, A, 10, 8, A, 1 << 20, None) == EINVAL                  # ldh < 2L
    assert l.gvf_posterior_fwd(A, 16, A, A, A, 0, 8, A, 1 << 20, None) == EINVAL                   # a mean over nothing
    assert l.gvf_posterior_fwd(A, 16, A, A, A, 4099, 8, A, 8, None) == EINVAL                      # workspace too small
    assert l.gvf_posterior_fwd(A, 16, A, A, A, 10, 8, ODD, 1 << 20, None) == EINVAL                # workspace not 8-byte aligned
    for hole in range(5):
        args = [A, 16, A, A, A, 10, 8, A, 1 << 20, None]
        args[(0, 2, 3, 4, 7)[hole]] = None
        assert l.gvf_posterior_fwd(*args) == EINVAL
    assert l.gvf_posterior_bwd(None, 16, A, A, A, A, 16, 10, 8, None) == EINVAL and l.gvf_posterior_bwd(A, 16, A, A, A, None, 16, 10, 8, None) == EINVAL
    assert l.gvf_posterior_bwd(A, 16, None, A, A, A, 16, 10, 8, None) == EINVAL                    # dz without eps
    assert l.gvf_posterior_bwd(A, 16, A, A, A, A, 15, 10, 8, None) == EINVAL and l.gvf_posterior_bwd(A, 16, A, A, A, A, 16, 10, 0, None) == EINVAL
    assert l.gvf_posterior_bwd(None, 16, None, None, None, None, 16, 0, 8, None) == _lib.GVF_OK
    # regularisers
    assert l.gvf_gaussian_reg_workspace_bytes(-1, ctypes.byref(nb)) == EINVAL and l.gvf_gaussian_reg_workspace_bytes(5, None) == EINVAL
    assert l.gvf_gaussian_reg_workspace_bytes(8264, ctypes.byref(nb)) == _lib.GVF_OK and nb.value == 2 * 8 * 9
    assert l.gvf_gaussian_reg_fwd(A, A, 0, 0.0, 0.0, 0.0, 0, A, A, A, 1 << 20, None) == EINVAL
    assert l.gvf_gaussian_reg_fwd(A, A, 5, 0.0, 0.0, 0.0, 2, A, A, A, 1 << 20, None) == EINVAL      # activation
    assert l.gvf_gaussian_reg_fwd(A, A, 5, 0.0, 0.0, -1.0, 0, A, A, A, 1 << 20, None) == EINVAL     # kappa
    assert l.gvf_gaussian_reg_fwd(A, A, 8264, 0.0, 0.0, 0.0, 0, A, A, A, 64, None) == EINVAL        # workspace
    for hole in (0, 1, 7, 8, 9):
        args = [A, A, 5, 0.0, 0.0, 0.0, 0, A, A, A, 1 << 20, None]
        args[hole] = None
        assert l.gvf_gaussian_reg_fwd(*args) == EINVAL
    assert l.gvf_gaussian_reg_bwd(None, A, 5, 0.0, 0.0, 0.0, 0, A, A, A, A, None) == EINVAL
    assert l.gvf_gaussian_reg_bwd(A, A, 5, 0.0, 0.0, 0.0, 0, A, A, None, A, None) == EINVAL         # dvol without dscaling
    assert l.gvf_gaussian_reg_bwd(A, A, 5, 0.0, 0.0, 0.0, 0, A, A, A, None, None) == EINVAL         # dopa without dopacity
    assert l.gvf_gaussian_reg_bwd(A, A, 5, 0.0, 0.0, 0.0, 0, None, None, None, None, None) == EINVAL
    assert l.gvf_gaussian_reg_bwd(A, A, 5, 0.0, 0.0, 0.0, 3, A, A, A, A, None) == EINVAL
    assert l.gvf_gaussian_reg_bwd(None, None, 0, 0.0, 0.0, 0.0, 0, None, None, None, None, None) == _lib.GVF_OK
    # column sums
    assert l.gvf_colsum_f32_workspace_bytes(-1, 8, ctypes.byref(nb)) == EINVAL and l.gvf_colsum_f32_workspace_bytes(4, 0, ctypes.byref(nb)) == EINVAL
    assert l.gvf_colsum_f32_workspace_bytes(65535 * 64 + 1, 8, ctypes.byref(nb)) == EINVAL and l.gvf_colsum_f32_workspace_bytes(4, 8, None) == EINVAL
    assert l.gvf_colsum_f32_workspace_bytes(130, 100, ctypes.byref(nb)) == _lib.GVF_OK and nb.value == 3 * 100 * 8
    assert l.gvf_colsum_f32(A, 0, 8, A, A, 1 << 20, None) == EINVAL and l.gvf_colsum_f32(A, 130, 100, A, A, 64, None) == EINVAL
    assert l.gvf_colsum_f32(None, 4, 8, A, A, 1 << 20, None) == EINVAL and l.gvf_colsum_f32(A, 4, 8, None, A, 1 << 20, None) == EINVAL
    assert l.gvf_colsum_f32(A, 4, 8, A, None, 1 << 20, None) == EINVAL and l.gvf_colsum_f32(A, 4, 8, A, ODD, 1 << 20, None) == EINVAL


def test_operators_refuse_cpu_tensors_and_bad_shapes():
    with pytest.raises(_lib.GvfError):
        S.colsum(torch.zeros((4, 8)))
    with pytest.raises(_lib.GvfError):
        S.bias_grad_tap(torch.zeros((4, 8)), torch.zeros(8))
    u = torch.zeros(8, dtype=torch.bfloat16)
    with pytest.raises(_lib.GvfError):
        S.gelu_tanh(u)
    with pytest.raises(_lib.GvfError):
        S.gather_rows(torch.zeros((4, 8)), torch.arange(4))
    with pytest.raises(_lib.GvfError):
        S.posterior(torch.zeros((4, 16)), torch.zeros((4, 8)))
    with pytest.raises(_lib.GvfError):
        S.gaussian_reg(torch.zeros((4, 3)), torch.zeros((4, 1)), 0.0, 0.0)


# ---- the formulas of the reference file against float64 autograd ------------------------------------------------------------------
def test_reference_formulas_equal_float64_autograd():
    g = torch.Generator().manual_seed(1)
    u = (torch.randn(300, generator=g, dtype=torch.float64) * 3).requires_grad_()
    da = torch.randn(300, generator=g, dtype=torch.float64)
    F.gelu(u, approximate="tanh").backward(da)
    got = R.gelu(u.detach(), da)
    assert R.rel_l2(got["a"], F.gelu(u.detach(), approximate="tanh")) < 1e-14 and R.rel_l2(got["du"], u.grad) < 1e-8    # (the dropped tail: 2e-8 of a term)
    h = torch.randn((37, 6), generator=g, dtype=torch.float64).requires_grad_()
    eps, dz = torch.randn((37, 3), generator=g, dtype=torch.float64), torch.randn((37, 3), generator=g, dtype=torch.float64)
    m, lv = h.chunk(2, dim=-1)
    z = m + torch.exp(0.5 * lv) * eps
    kl = 0.5 * torch.mean(m.pow(2) + lv.exp() - lv - 1)
    ((z * dz).sum() + 0.7 * kl).backward()
    got = R.posterior(h.detach(), eps, dz, 0.7)
    assert R.rel_l2(got["z"], z.detach()) < 1e-14 and abs(float(got["kl"] - kl.detach())) < 1e-14 and R.rel_l2(got["dh"], h.grad) < 1e-13
    for softplus in (False, True):
        for kappa in (0.0, 9e-4):
            s = (torch.randn((50, 3), generator=g, dtype=torch.float64) * 2)
            s[:5] += 22.0                                        # the linear branch of the softplus
            s.requires_grad_()
            o = torch.randn(50, generator=g, dtype=torch.float64).requires_grad_()
            a = F.softplus(s + 0.3) if softplus else torch.exp(s + 0.3)
            vol = torch.sqrt(a * a + kappa ** 2).prod(dim=1).mean()
            opa = (torch.sigmoid(o - 0.2) - 1).pow(2).mean()
            (1.5 * vol - 0.5 * opa).backward()
            got = R.reg(s.detach(), o.detach(), 0.3, -0.2, kappa, softplus, 1.5, -0.5)
            vol, opa = vol.detach(), opa.detach()
            assert abs(float(got["vol"] - vol)) <= 1e-13 * float(vol) and abs(float(got["opa"] - opa)) < 1e-14
            assert R.rel_l2(got["ds"], s.grad) < 1e-12 and R.rel_l2(got["do"], o.grad) < 1e-12


# ---- the switch -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gold():
    return R.golden()


def _model(cfg, sd, **kw):
    m = SparseTransformerVAE(**dict(cfg, **kw))
    m.load_state_dict(sd, strict=True)
    return m


def test_enable_training_is_an_explicit_switch(gold):
    cfg, sd, feats, coords, noise, W = gold
    m = _model(cfg, sd)
    x = sp.SparseTensor(feats, coords)
    assert not m.training_enabled()
    m.train()                                                    # not keyed on self.training ...
    assert not m.training_enabled() and not m._train_now()
    assert all(p.requires_grad for p in m.parameters())          # ... nor on requires_grad: the inference path refuses the CPU tensor
    with pytest.raises(_lib.GvfError):
        m.encode(x)
    assert m.enable_training() is m and m.training_enabled() and m._train_now()
    with torch.no_grad():                                        # under no_grad the call is the inference path again
        assert not m._train_now()
        with pytest.raises(_lib.GvfError):
            m.encode(x)
    with pytest.raises(_lib.GvfError):                           # on, with grad, HIP operators: CPU tensors are refused, no fallback
        m(x, noise=noise)
    with pytest.raises(ValueError):
        m.enable_training(dtype=torch.float32)                   # the HIP operators are 16-bit
    m.enable_training(False)
    assert not m.training_enabled()
    with pytest.raises(RuntimeError, match="enable_training"):
        m(x, return_kl=True)


def test_training_losses_errors(gold):
    cfg, sd, feats, coords, noise, W = gold
    m = _model(cfg, sd)
    vae = SparseVAE({"vae": m}, resolution=cfg["resolution"], representation_config={"MipGS": {}}, lambda_lpips=0.2)
    x = sp.SparseTensor(feats, coords)
    img, cam = torch.zeros((2, 3, 16, 16)), torch.eye(4)[None].repeat(2, 1, 1)
    with pytest.raises(RuntimeError, match=r"enable_training\(\)"):
        vae.training_losses(x, img, cam, cam[:, :3, :3])
    m.enable_training()
    with pytest.raises(ValueError, match="lpips"):
        vae.training_losses(x, img, cam, cam[:, :3, :3])
    from gvfdiffusion_amd import training
    with pytest.raises(ValueError, match="lpips"):
        training.static_vae_loss(vae, x, img, cam, cam[:, :3, :3])


# ---- the wiring: TorchOps in fp32 on the CPU against float64 autograd of the oracle ---------------------------------------------------
@pytest.fixture(scope="module")
def ref64(gold):
    return R.golden_loss(*gold)


def _grads(m, feats, coords, noise, W):
    x = sp.SparseTensor(feats.clone().requires_grad_(), coords)
    loss, out = R.model_loss(m, x, noise, W)
    names, params = zip(*m.named_parameters())
    g = torch.autograd.grad(loss, list(params) + [x.feats])
    return loss.detach(), out, dict(zip(names + ("feats",), g))


def test_training_forward_through_torch_ops_matches_float64_oracle(gold, ref64):
    """Every parameter's gradient and the feature gradient within 1e-5 relative L2 of float64 autograd of the oracle (the bar of
    tests/test_dit_train_host.py; the oracle's own fp32 run measures 5.5e-7 here), and the same gradients under use_checkpoint."""
    cfg, sd, feats, coords, noise, W = gold
    loss64, out64, g64 = ref64
    m = _model(cfg, sd).enable_training(dtype=torch.float32, ops=R.TorchOps())
    loss, out, g = _grads(m, feats, coords, noise, W)
    assert out.feats.dtype == torch.float32 and out.feats.grad_fn is not None
    assert abs(float(loss) - float(loss64)) <= 1e-5 * abs(float(loss64)) and R.rel_l2(out.feats.detach(), out64) <= 1e-5
    assert set(g) == set(g64)
    worst = 0.0
    for k in g:
        assert g64[k] is not None and float(g64[k].abs().max()) > 0, f"{k}: the reference gradient is zero"
        e = R.rel_l2(g[k], g64[k])
        worst = max(worst, e)
        assert e <= 1e-5, f"{k}: rel L2 {e:.3e}"
    print(f"torch-ops fp32 wiring: worst gradient rel L2 {worst:.2e}")
    mc = _model(cfg, sd, use_checkpoint=True).enable_training(dtype=torch.float32, ops=R.TorchOps())
    assert all(b.use_checkpoint for b in list(mc.encoder) + list(mc.decoder))
    _, _, gc = _grads(mc, feats, coords, noise, W)
    for k in g:
        assert torch.equal(g[k], gc[k]), f"{k}: use_checkpoint changed the gradient"


def test_block_both_qkv_layouts_full_attention_through_torch_ops(gold):
    """full attention (no gather) and the [q|k|v][head][c] layout reach the same operators: one block through TorchOps against the oracle's
    block in float64 (the serialisation order is computed on the device: tests/test_sparse_vae_train_gpu.py)."""
    from gvfdiffusion_amd.model.sparse_voxel_diffusion import SparseTransformerBlock
    from oracle import sparse_vae_ref as ref
    cfg, sd, feats, coords, noise, W = gold
    C, H = cfg["model_channels"], cfg["num_heads"]
    x = torch.randn((coords.shape[0], C), generator=torch.Generator().manual_seed(3))
    st = sp.SparseTensor(x, coords)
    bsd = {k[len("encoder.0."):]: v for k, v in sd.items() if k.startswith("encoder.0.")}
    for old in (True, False):
        blk = SparseTransformerBlock(C, num_heads=H, attn_mode="full", modulated=False, use_old_attn_impl=old)
        blk.load_state_dict(bsd)
        xr = x.clone().requires_grad_()
        y = blk.forward_rows_train(xr, st, torch.float32, ops=R.TorchOps())
        x64 = x.double().requires_grad_()
        y64 = ref.block(x64, coords[:, 0].long(), {"b." + k: v.double() for k, v in bsd.items()}, "b", H, "fp32", old)
        assert R.rel_l2(y.detach(), y64.detach()) <= 1e-5
        w = torch.randn(y.shape, generator=torch.Generator().manual_seed(4))
        gx, = torch.autograd.grad((y * w).sum(), xr)
        g64, = torch.autograd.grad((y64 * w.double()).sum(), x64)
        assert R.rel_l2(gx, g64) <= 1e-5
