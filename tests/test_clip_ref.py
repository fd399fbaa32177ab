"""The float64 restatement of CLIP's image tower (tests/clip_ref.py) -- the reference the GPU tests hold the HIP encoder to -- against an
implementation nobody here wrote: transformers' CLIPVisionModelWithProjection, built from a config (no download), in float64.  stream =
last_hidden_state, feat = image_embeds; agreement to 1e-10.  Every mutant of the restatement (one wrong decision each) must fall outside
that by a factor 1e3.  Plus the preprocessing constants, the state-dict names of the HIP module and the preprocessing restatement.  No GPU."""
import functools

import numpy as np
import pytest
import torch

import clip_ref as C

D, DEPTH, GRID, E = 128, 2, 2, 64          # hidden 128 = 2 heads of 64, image 64 x 64, patch 32
TOL = 1e-10


def hf_model():
    tr = pytest.importorskip("transformers")
    cfg = tr.CLIPVisionConfig(hidden_size=D, intermediate_size=4 * D, num_hidden_layers=DEPTH, num_attention_heads=D // 64, image_size=GRID * 32,
                              patch_size=32, projection_dim=E, hidden_act="quick_gelu", layer_norm_eps=1e-5, attention_dropout=0.0)
    return tr.CLIPVisionModelWithProjection(cfg).double().eval()


@functools.lru_cache(maxsize=None)
def _case():
    sd = C.random_state_dict(D, DEPTH, GRID, E, seed=3)
    model = hf_model()
    res = model.load_state_dict({k: v.double() for k, v in C.to_hf(sd).items()}, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    pix = C.normalise_u8(torch.randint(0, 256, (2, 3, GRID * 32, GRID * 32), generator=torch.Generator().manual_seed(5), dtype=torch.uint8),
                         torch.float64)
    with torch.no_grad():
        o = model(pixel_values=pix)
    return sd, model, pix, o.last_hidden_state, o.image_embeds


def _errs(out, stream, feat):
    return float((out["stream"] - stream).abs().max()), float((out["feat"] - feat).abs().max())


def test_restatement_agrees_with_transformers():
    sd, _, pix, stream, feat = _case()
    out = C.forward(sd, pix)
    assert out["stream"].shape == (2, 1 + GRID * GRID, D) and out["feat"].shape == (2, E)
    e_s, e_f = _errs(out, stream, feat)
    print(f"max |restatement - transformers|: last_hidden_state {e_s:.2e}, image_embeds {e_f:.2e}")
    assert e_s <= TOL and e_f <= TOL


@pytest.mark.parametrize("mutant", C.MUTANTS)
def test_comparison_rejects_mutants(mutant):
    sd, _, pix, stream, feat = _case()
    e_s, e_f = _errs(C.forward(sd, pix, mutant=mutant), stream, feat)
    print(f"mutant {mutant}: max |mutant - transformers|: last_hidden_state {e_s:.2e}, image_embeds {e_f:.2e}")
    assert max(e_s, e_f) > 1e3 * TOL


def test_preprocessing_constants():
    iu = pytest.importorskip("transformers.image_utils")
    from gvfdiffusion_amd.ops import clip as clip_ops
    assert list(C.CLIP_MEAN) == list(iu.OPENAI_CLIP_MEAN) and list(C.CLIP_STD) == list(iu.OPENAI_CLIP_STD)
    assert tuple(clip_ops.CLIP_MEAN) == C.CLIP_MEAN and tuple(clip_ops.CLIP_STD) == C.CLIP_STD
    for dt in (torch.float16, torch.bfloat16):
        t = clip_ops.operand_table(dt)
        assert t.dtype == dt and t.shape == (3, 256) and torch.equal(t.view(torch.int16), C.operand_table(dt).view(torch.int16))
    # fp16: the table IS ToTensor -> Normalize -> .half() of every pixel value
    u8 = torch.arange(256, dtype=torch.uint8).view(1, 1, 16, 16).repeat(1, 3, 1, 1)
    assert torch.equal(clip_ops.operand_table(torch.float16).view(3, 16, 16)[None], C.normalise_u8(u8).half())


def test_module_state_dict_names_and_the_three_input_forms():
    from gvfdiffusion_amd.model.clip import CLIPVisionTransformer, clip_vit_b32, load_clip_state_dict
    listed = ["conv1.weight", "class_embedding", "positional_embedding", "ln_pre.weight", "ln_pre.bias", "ln_post.weight", "ln_post.bias", "proj"]
    for i in range(DEPTH):
        listed += [f"transformer.resblocks.{i}.{n}" for n in ("ln_1.weight", "ln_1.bias", "attn.in_proj_weight", "attn.in_proj_bias",
                                                              "attn.out_proj.weight", "attn.out_proj.bias", "ln_2.weight", "ln_2.bias",
                                                              "mlp.c_fc.weight", "mlp.c_fc.bias", "mlp.c_proj.weight", "mlp.c_proj.bias")]
    mk = lambda: CLIPVisionTransformer(input_resolution=GRID * 32, patch_size=32, width=D, layers=DEPTH, heads=D // 64, output_dim=E)
    m = mk()
    assert list(m.state_dict().keys()) == C.state_dict_keys(DEPTH) and set(m.state_dict().keys()) == set(listed)
    sd = C.random_state_dict(D, DEPTH, GRID, E)
    shapes = {k: tuple(v.shape) for k, v in sd.items()}
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == shapes
    same = lambda mod: all(torch.equal(mod.state_dict()[k], v) for k, v in sd.items())
    assert same(load_clip_state_dict(mk(), sd))                                                       # OpenAI's model.visual dict
    full = {"visual." + k: v for k, v in sd.items()}
    full.update({"logit_scale": torch.zeros(()), "token_embedding.weight": torch.zeros(4, 8), "transformer.resblocks.0.ln_1.weight": torch.zeros(8)})
    assert same(load_clip_state_dict(mk(), full))                                                     # a full CLIP dict: the text tower is ignored
    assert same(load_clip_state_dict(mk(), C.to_hf(sd)))                                              # transformers' names
    hf = hf_model()                                                                                   # ... and back: strict in both directions
    res = hf.load_state_dict({k: v.double() for k, v in C.to_hf(sd).items()}, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert same(load_clip_state_dict(mk(), {k: v.float() for k, v in hf.state_dict().items()}))
    for bad in (dict(sd, extra=torch.zeros(1)), {k: v for k, v in sd.items() if k != "proj"}, dict(C.to_hf(sd), **{"vision_model.extra": torch.zeros(1)})):
        with pytest.raises(RuntimeError):
            load_clip_state_dict(mk(), bad)
    for kw in (dict(patch_size=16), dict(width=96, heads=2), dict(width=128, heads=4), dict(input_resolution=100), dict(output_dim=100)):
        with pytest.raises(NotImplementedError):
            CLIPVisionTransformer(**{**dict(input_resolution=64, patch_size=32, width=D, layers=1, heads=2, output_dim=E), **kw})
    with pytest.raises(NotImplementedError):
        m.train()
    import inspect
    assert "pretrained" not in inspect.signature(clip_vit_b32).parameters


def test_vit_b32_factory_has_the_released_shapes():
    from gvfdiffusion_amd.model.clip import clip_vit_b32
    with torch.device("meta"):
        m = clip_vit_b32()
    sd = m.state_dict()
    assert sd["positional_embedding"].shape == (50, 768) and sd["conv1.weight"].shape == (768, 3, 32, 32) and sd["proj"].shape == (768, 512)
    assert len(m.transformer.resblocks) == 12 and sd["transformer.resblocks.11.mlp.c_fc.weight"].shape == (3072, 768)
    assert sd["transformer.resblocks.0.attn.in_proj_weight"].shape == (2304, 768) and "conv1.bias" not in sd


@pytest.mark.parametrize("S", [512, 300])
def test_preprocessing_restatement_is_the_clip_image_processor(S):
    """numpy truncation + PIL bicubic resize to 224 x 224 == transformers' PIL CLIP image processor with rescaling and normalisation off."""
    tr = pytest.importorskip("transformers")
    pytest.importorskip("PIL.Image")
    from PIL import Image
    try:
        from transformers.models.clip.image_processing_pil_clip import CLIPImageProcessorPil as Proc
    except ImportError:
        Proc = tr.CLIPImageProcessor
    proc = Proc(do_rescale=False, do_normalize=False)
    g = torch.Generator().manual_seed(S)
    u8 = torch.randint(0, 256, (2, 3, S, S), generator=g, dtype=torch.uint8)
    ours = C.preprocess_u8(_exact01(u8))
    pil = [Image.fromarray(np.ascontiguousarray(f.permute(1, 2, 0).numpy())) for f in u8]
    theirs = np.asarray(proc(images=pil, return_tensors="np")["pixel_values"])
    assert theirs.shape == (2, 3, 224, 224)
    assert np.array_equal(theirs.astype(np.float64), ours.numpy().astype(np.float64))


def _exact01(u8):
    """fp32 images in [0, 1] whose x * 255 truncates back to u8: (u8 + 0.5) / 255."""
    x = (u8.float() + 0.5) / 255.0
    assert torch.equal(x.mul(255).to(torch.uint8), u8)
    return x


def test_truncation_is_not_rounding():
    img = torch.rand((2, 3, 300, 300), generator=torch.Generator().manual_seed(9))
    a, b = C.preprocess_u8(img), C.preprocess_u8(img, rounding=True)
    assert a.shape == b.shape == (2, 3, 224, 224) and not torch.equal(a, b)
    assert not torch.equal(img.mul(255).to(torch.uint8), img.mul(255).round().to(torch.uint8))


def test_inference_script_takes_a_local_clip_checkpoint(tmp_path):
    import inference_dpm_latent as S
    a = S.create_argparser().parse_args(["--synthetic", "--clip_ckpt", "ViT-B-32.pt"])
    assert a.clip_ckpt == "ViT-B-32.pt" and S.clip_encoder(S.create_argparser().parse_args(["--synthetic"]), torch.device("cpu")) is None
    for bad in ("https://example.invalid/ViT-B-32.pt", str(tmp_path / "missing.pt")):
        with pytest.raises(SystemExit):
            S.clip_encoder(S.create_argparser().parse_args(["--synthetic", "--clip_ckpt", bad]), torch.device("cpu"))
