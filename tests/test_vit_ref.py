"""The float64 restatement of the DINOv2 ViT (tests/vit_ref.py) -- the reference the GPU tests hold the image encoder to -- against an
implementation nobody here wrote: transformers' Dinov2WithRegistersModel / Dinov2Model, built from a config (no download), in float64.
x_prenorm = hidden_states[-1], x_norm = last_hidden_state; agreement to 1e-10.  Every mutant of the restatement (one wrong decision each)
must fall outside that.  Plus the state-dict names of the HIP module.  No GPU."""
import functools

import pytest
import torch

import vit_ref as V

D, DEPTH, GRID = 128, 2, 4          # hidden 128 = 2 heads of 64, image 56 x 56
TOL = 1e-10


def hf_model(R):
    tr = pytest.importorskip("transformers")
    kw = dict(hidden_size=D, num_hidden_layers=DEPTH, num_attention_heads=D // 64, image_size=GRID * 14, patch_size=14, mlp_ratio=4,
              hidden_act="gelu", layer_norm_eps=1e-6, qkv_bias=True, use_swiglu_ffn=False, hidden_dropout_prob=0.0,
              attention_probs_dropout_prob=0.0, drop_path_rate=0.0)
    if R:
        model = tr.Dinov2WithRegistersModel(tr.Dinov2WithRegistersConfig(num_register_tokens=R, **kw))
    else:
        model = tr.Dinov2Model(tr.Dinov2Config(**kw))
    return model.double().eval()


@functools.lru_cache(maxsize=None)
def _case(R):
    sd = V.random_state_dict(D, DEPTH, GRID, R, seed=3)
    model = hf_model(R)
    missing = model.load_state_dict({k: v.double() for k, v in V.to_hf(sd).items()}, strict=True)
    assert not missing.missing_keys and not missing.unexpected_keys
    img = torch.rand((2, 3, GRID * 14, GRID * 14), generator=torch.Generator().manual_seed(5))
    return R, sd, model, img


def hf_run(model, pixel_values):
    with torch.no_grad():
        o = model(pixel_values=pixel_values, output_hidden_states=True)
    return o.hidden_states[-1], o.last_hidden_state


@pytest.mark.parametrize("R", [4, 0])
def test_restatement_agrees_with_transformers(R):
    R, sd, model, img = _case(R)
    pre, norm = hf_run(model, V.zscore(img, torch.float64))
    out = V.forward(sd, img, R)
    assert out["x_prenorm"].shape == (2, 1 + R + GRID * GRID, D)
    e_pre, e_norm = float((out["x_prenorm"] - pre).abs().max()), float((out["x_norm"] - norm).abs().max())
    print(f"R={R}: max |restatement - transformers|: x_prenorm {e_pre:.2e}, x_norm {e_norm:.2e}")
    assert e_pre <= TOL and e_norm <= TOL
    # the TRELLIS read-out is F.layer_norm of x_prenorm (trellis_image_to_3d.py:142-146)
    assert torch.equal(out["trellis"], torch.nn.functional.layer_norm(out["x_prenorm"], (D,)))


@pytest.mark.parametrize("R,mutant", [(R, m) for R in (4, 0) for m in V.MUTANTS if m != "zscore_after_rounding" and not (m == "reg_pos" and R == 0)])
def test_comparison_rejects_mutants(R, mutant):
    R, sd, model, img = _case(R)
    pre, _ = hf_run(model, V.zscore(img, torch.float64))
    e = float((V.forward(sd, img, R, mutant=mutant)["x_prenorm"] - pre).abs().max())
    print(f"R={R} mutant {mutant}: max |mutant - transformers| = {e:.2e}")
    assert e > 1e3 * TOL


@pytest.mark.parametrize("R", [4, 0])
@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def test_operand_rounding_point(R, dt):
    """The 16-bit operand of the patch convolution is the fp32 z-score rounded once: the restatement with operand_dtype equals transformers fed
    those rounded normalised pixels and the rounded weight; z-scoring the rounded pixels instead is a different model."""
    R, sd, model, img = _case(R)
    sd16 = dict(sd)
    sd16["patch_embed.proj.weight"] = sd["patch_embed.proj.weight"].to(dt).float()
    m16 = hf_model(R)
    m16.load_state_dict({k: v.double() for k, v in V.to_hf(sd16).items()}, strict=True)
    pre, _ = hf_run(m16, V.patch_operand(img, dt))
    good = float((V.forward(sd, img, R, operand_dtype=dt)["x_prenorm"] - pre).abs().max())
    bad = float((V.forward(sd, img, R, operand_dtype=dt, mutant="zscore_after_rounding")["x_prenorm"] - pre).abs().max())
    print(f"R={R} {dt}: rounded z-score {good:.2e}, z-score of rounded pixels {bad:.2e}")
    assert good <= TOL and bad > 1e3 * TOL


def test_patch_rows_match_the_convolution():
    """patch_rows' column order is the conv weight's own flattening: rows @ W.T == F.conv2d."""
    g = torch.Generator().manual_seed(1)
    a = torch.randn((2, 3, 42, 28), generator=g, dtype=torch.float64)
    w = torch.randn((8, 3, 14, 14), generator=g, dtype=torch.float64)
    conv = torch.nn.functional.conv2d(a, w, stride=14).flatten(2).transpose(1, 2).reshape(-1, 8)
    assert float((V.patch_rows(a) @ w.reshape(8, -1).T - conv).abs().max()) < 1e-12


@pytest.mark.parametrize("R", [4, 0])
def test_module_state_dict_names(R):
    from gvfdiffusion_amd.model.dinov2 import DinoVisionTransformer, dinov2_vitl14_reg, dinov2_vitl14
    m = DinoVisionTransformer(img_size=GRID * 14, patch_size=14, embed_dim=D, depth=DEPTH, num_heads=D // 64, num_register_tokens=R, init_values=1.0)
    assert list(m.state_dict().keys()) == V.state_dict_keys(DEPTH, R)
    assert m.num_register_tokens == R
    sd = V.random_state_dict(D, DEPTH, GRID, R)
    m.load_state_dict(sd, strict=True)
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == {k: tuple(v.shape) for k, v in sd.items()}
    for kw in (dict(ffn_layer="swiglufused"), dict(drop_path_rate=0.1), dict(init_values=None)):
        with pytest.raises(NotImplementedError):
            DinoVisionTransformer(img_size=56, embed_dim=D, depth=1, num_heads=2, **kw)
    with pytest.raises(NotImplementedError):
        m.train()
    with pytest.raises(NotImplementedError):
        m(torch.zeros(1, 3, 56, 56), masks=torch.zeros(1, 16, dtype=torch.bool))
    import inspect
    for f in (dinov2_vitl14_reg, dinov2_vitl14):
        assert "pretrained" not in inspect.signature(f).parameters


def test_vitl_factories_have_the_released_shapes():
    from gvfdiffusion_amd.model.dinov2 import dinov2_vitl14_reg
    with torch.device("meta"):
        m = dinov2_vitl14_reg()
    sd = m.state_dict()
    assert sd["pos_embed"].shape == (1, 1370, 1024) and sd["register_tokens"].shape == (1, 4, 1024) and len(m.blocks) == 24
    assert sd["blocks.23.mlp.fc1.weight"].shape == (4096, 1024) and sd["patch_embed.proj.weight"].shape == (1024, 3, 14, 14)


def test_inference_script_takes_cond_frames():
    import inference_dpm_latent as S
    a = S.create_argparser().parse_args(["--synthetic", "--cond_frames", "frames.pt", "--dinov2_ckpt", "vitl14_reg.pth"])
    assert a.cond_frames == "frames.pt" and a.dinov2_ckpt == "vitl14_reg.pth" and a.cond_images is None
    with pytest.raises(SystemExit):                                      # neither a checkpoint nor --synthetic: no silent random encoder
        S.image_encoder(S.create_argparser().parse_args(["--cond_frames", "frames.pt"]), torch.device("cpu"))
