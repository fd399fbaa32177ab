"""The DiT forward's call plan (model/dit_plan.py), pinned on the host: DiT.forward_plan on CPU models, field by field.  Every expected value
is written out by hand from the rules ("which launches a forward makes"); no second implementation of the rules is
called, no library is loaded, no GPU is needed.  tests/test_dit_plan_gpu.py checks on the device that the plan is what runs."""
import json
import os

import numpy as np
import pytest

from gvfdiffusion_amd.model import dit_plan
from gvfdiffusion_amd.model.dit import DiT

GOLD = os.path.join(os.path.dirname(__file__), "golden")
MAN = json.load(open(os.path.join(GOLD, "dit_manifest.json")))
C, H, NB = 512, 16, 2
ZERO = dict.fromkeys(dit_plan.LAUNCH_NAMES, 0)


def net(**over):
    """Manifest configuration (C = 512, 16 heads of 32, Cin = Cout = 16, MLP 2048, temporal attention) with two blocks; keywords that name a
    switch attribute are assigned, the others go to the constructor."""
    switches = {k: over.pop(k) for k in list(over) if k in ("use_rowblock", "rowblock_tiled_kv", "rowblock_temporal", "weight_prefetch",
                                                            "fuse_layernorm", "modulation_table")}
    m = DiT(**dict(MAN["config"], num_blocks=NB, **over))
    for k, v in switches.items():
        setattr(m, k, v)
    return m


@pytest.fixture(scope="module")
def base():
    return net()


def rowblock_launches(fused, tiled, pack, attention):
    return dict(ZERO, rowblock_fused=fused, attention_tiled=tiled, attention_pack_kv=pack, attention=attention, final_layer_f32=1)


# per block without the folded LayerNorm: 5 LayerNorm launches (to_qkv x 2, to_q x 2, mlp.0), each followed by its GEMM, and 5 residual GEMMs;
# the spatial attention packs its K / V and runs tiled like the two cross attentions, the temporal one is csrc/attn.hip's
UNFUSED = dict(ZERO, gemm=20, layernorm_modulate=10, attention_tiled=6, attention_pack_kv=2, attention=2, input_layer_f32=1, final_layer_f32=1)


def test_whole_blocks_without_key_tiles_every_field(base):
    """(T, N) = (3, 48), B = 2: 144 rows per sample = 3 whole blocks; 48 is no multiple of 64, so to_qkv stays row-major and is packed;
    3 | 48, so the temporal attention runs inside the row-block launch."""
    p = base.forward_plan(2, 3, 48)
    assert (p.path, p.small_f32, p.mod_f32, p.TN, p.TNp, p.padded, p.M) == ("rowblock", True, True, 144, 144, False, 288)
    assert (p.tiled_kv, p.temporal_fused, p.prefetch) == (False, True, True)
    assert (p.fuse_ln, p.strided_attention) == (False, False)
    assert p.streams == ("s23", "s4", "s5") and p.spatial_prefetch_stream is None        # the packed path's spatial attention prefetches nothing
    assert p.attention_workgroups == NB * 3 * 2 * 3 * H * 1
    assert dict(p.launches) == rowblock_launches(7, 6, 2, 0)
    assert dict(p.modulation_launches) == {"timestep_embed_f32": 1, "modulation_f32": 1}
    # the unpadded frame views: all B T frames as one uniform run, one key set per frame
    assert tuple(p.frames) == ((6, 1), (48 * C, 0, C), (48 * 3 * C, 0, 3 * C), (1, 0), (144 * C, 48 * C, C))


@pytest.mark.parametrize("T, N, padded, TNp, tiled, fused, launches", [
    (3, 64, False, 192, True, True, rowblock_launches(7, 6, 0, 0)),
    (5, 48, False, 240, False, False, rowblock_launches(9, 6, 2, 2)),
    (5, 64, True, 336, True, False, rowblock_launches(9, 6, 0, 2)),
    (16, 512, True, 8208, True, True, rowblock_launches(7, 6, 0, 0)),
    (24, 512, False, 12288, True, True, rowblock_launches(7, 6, 0, 0)),
    (32, 512, True, 16416, True, False, rowblock_launches(9, 6, 0, 2)),
])
def test_rowblock_shapes(base, T, N, padded, TNp, tiled, fused, launches):
    p = base.forward_plan(1, T, N)
    assert p.path == "rowblock"
    assert (p.padded, p.TN, p.TNp, p.M, p.tiled_kv, p.temporal_fused) == (padded, T * N, TNp, TNp, tiled, fused)
    assert p.streams == (("s23", "s4", "s5") if fused else ("s2", "s3", "s4", "s5"))
    assert p.spatial_prefetch_stream == (None if not tiled else "s23" if fused else "s2")
    assert dict(p.launches) == launches


def test_released_shape(base):
    full = DiT(**MAN["config"])
    for B in (1, 3):
        p = full.forward_plan(B, 24, 512)
        assert p.path == "rowblock" and not p.padded and p.streams == ("s23", "s4", "s5")
        assert p.attention_workgroups == 12 * 3 * B * 24 * 16 * ((512 + 255) // 256) == full.attention_workgroups(B, 24, 512)
        assert dict(p.launches) == rowblock_launches(37, 36, 0, 0)
    assert base.forward_plan(1, 24, 512).attention_workgroups == NB * 3 * 24 * 16 * 2


def test_padded_frame_views(base):
    """(5, 64) at B = 3: outer = sample (stride TNp rows), inner = frame (N rows), key set of (b, f) = b T + f."""
    p = base.forward_plan(3, 5, 64)
    assert p.padded and p.M == 3 * 336
    assert tuple(p.frames) == ((3, 5), (336 * C, 64 * C, C), (336 * 3 * C, 64 * 3 * C, 3 * C), (5, 1), (336 * C, 64 * C, C))


def test_shapes_and_switches_that_leave_the_rowblock_path(base):
    for p in (base.forward_plan(1, 5, 40),                                      # would be padded (200 -> 240 rows) and 40 is no multiple of 64
              net(rowblock_tiled_kv=False).forward_plan(1, 5, 64),              # padded needs the tiled K / V epilogue
              net(use_rowblock=False).forward_plan(1, 3, 64)):
        assert p.path == "unfused" and not p.padded and p.TNp == p.TN == p.M and p.frames is None and p.streams == ()
        assert not p.tiled_kv and not p.temporal_fused and not p.prefetch and p.spatial_prefetch_stream is None
        assert p.small_f32 and not p.strided_attention and not p.fuse_ln
        assert dict(p.launches) == UNFUSED


def test_switches_inside_the_rowblock_path():
    p = net(rowblock_temporal=False).forward_plan(1, 3, 64)
    assert p.path == "rowblock" and not p.temporal_fused and p.streams == ("s2", "s3", "s4", "s5") and p.spatial_prefetch_stream == "s2"
    assert dict(p.launches) == rowblock_launches(9, 6, 0, 2)
    p = net(rowblock_tiled_kv=False).forward_plan(1, 3, 64)                     # unpadded: stays on the path, packs K / V with its own launch
    assert p.path == "rowblock" and not p.tiled_kv and p.spatial_prefetch_stream is None and dict(p.launches) == rowblock_launches(7, 6, 2, 0)
    p = net(weight_prefetch=False).forward_plan(1, 3, 64)
    assert p.path == "rowblock" and not p.prefetch and p.spatial_prefetch_stream == "s23"


def test_without_temporal_attention():
    p = net(no_temporal_attn=True).forward_plan(1, 2, 96)
    assert p.path == "rowblock" and not p.padded and not p.tiled_kv and not p.temporal_fused
    assert p.streams == ("s2", "s4", "s5") and dict(p.launches) == rowblock_launches(7, 6, 2, 0)


def test_layernorm_folded_into_the_gemms():
    """(1, 128): 128 rows, C = 512: the fold applies.  The fp32 input layer writes no row statistics, so block 0's to_qkv keeps its LayerNorm
    launch; mode 1 folds the other 9 projections, mode 2 only the 4 that are at most 512 wide (to_q of the cross attentions)."""
    p = net(use_rowblock=False, fuse_layernorm=1).forward_plan(1, 1, 128)
    assert p.path == "unfused" and p.fuse_ln and p.fuse_max_n == 1 << 30
    assert dict(p.launches) == dict(UNFUSED, gemm=1, layernorm_modulate=1, gemm_ln_bf16=9, gemm_resid_stats=10)
    p = net(use_rowblock=False, fuse_layernorm=2).forward_plan(1, 1, 128)
    assert p.fuse_ln and p.fuse_max_n == 512
    assert dict(p.launches) == dict(UNFUSED, gemm=6, layernorm_modulate=6, gemm_ln_bf16=4, gemm_resid_stats=10)
    assert not net(use_rowblock=False, fuse_layernorm=1).forward_plan(1, 1, 64).fuse_ln       # 64 rows: no multiple of 128
    assert not net(fuse_layernorm=1).forward_plan(1, 1, 128).fuse_ln                          # the row-block path has no such GEMMs


def test_geometries_the_rowblock_launch_does_not_cover():
    p = net(num_heads=8).forward_plan(1, 3, 64)                                 # heads of 64: strided flash attention for all four sub-layers
    assert p.path == "unfused" and p.strided_attention and p.small_f32
    assert dict(p.launches) == dict(UNFUSED, attention=8, attention_tiled=0, attention_pack_kv=0)
    g = np.load(os.path.join(GOLD, "dit_small_golden.npz"))
    small = DiT(**json.loads(bytes(g["cfg_json"]).decode()))                    # C = 64
    p = small.forward_plan(*g["x"].shape[:3])
    assert p.path == "unfused" and p.small_f32 and p.mod_f32
    p = net(model_channels=768, num_heads=24).forward_plan(1, 3, 64)            # above 512 channels the two small projections are 16-bit GEMMs
    assert p.path == "unfused" and not p.small_f32 and p.mod_f32
    assert dict(p.launches) == dict(UNFUSED, gemm=22, layernorm_modulate=11, cast_pad=1, input_layer_f32=0, final_layer_f32=0)
    p = net(in_channels=7).forward_plan(1, 3, 64)                               # the row-block input layer reads x in 16-byte pieces
    assert p.path == "unfused" and p.small_f32 and dict(p.launches) == UNFUSED
    p = net(model_channels=1280, num_heads=40).forward_plan(1, 3, 64)           # wider than the fp32 modulation kernels: three 16-bit GEMMs
    assert not p.mod_f32 and dict(p.modulation_launches) == {"cast_pad": 3, "gemm": 3}


ENV = {"GVF_DIT_ROWBLOCK": "rowblock", "GVF_DIT_TILED_KV": "tiled_kv", "GVF_DIT_TEMPORAL_FUSED": "temporal_fused", "GVF_DIT_PREFETCH": "prefetch",
       "GVF_DIT_MODTABLE": "modtable"}


def test_switches_from_the_environment(monkeypatch):
    for name in list(ENV) + ["GVF_DIT_FUSE_LN"]:
        monkeypatch.delenv(name, raising=False)
    default = dit_plan.DiTSwitches(rowblock=True, tiled_kv=True, temporal_fused=True, prefetch=True, fuse_ln=0, modtable=True)
    assert dit_plan.DiTSwitches.from_env() == default == dit_plan.DiTSwitches()
    for name, field in ENV.items():
        monkeypatch.setenv(name, "0")
        assert dit_plan.DiTSwitches.from_env() == default._replace(**{field: False})
        monkeypatch.setenv(name, "1")
        assert dit_plan.DiTSwitches.from_env() == default
        monkeypatch.delenv(name)
    for v in (1, 2):
        monkeypatch.setenv("GVF_DIT_FUSE_LN", str(v))
        assert dit_plan.DiTSwitches.from_env() == default._replace(fuse_ln=v)
    # the constructor reads it once into the writable attributes
    monkeypatch.setenv("GVF_DIT_ROWBLOCK", "0")
    m = net()
    assert (m.use_rowblock, m.rowblock_tiled_kv, m.rowblock_temporal, m.weight_prefetch, m.fuse_layernorm, m.modulation_table) == \
        (False, True, True, True, 2, True)
    monkeypatch.delenv("GVF_DIT_ROWBLOCK")
    assert m.forward_plan(1, 3, 64).path == "unfused"                           # ... and later changes of the environment do not reach it


def test_plan_is_memoised_hashable_and_follows_the_attributes(base):
    p = base.forward_plan(1, 3, 64)
    assert base.forward_plan(1, 3, 64) is p and net().forward_plan(1, 3, 64) is p           # equal inputs: the same object
    assert hash(p) == hash(base.forward_plan(1, 3, 64)) and p != base.forward_plan(1, 3, 48)
    with pytest.raises(Exception):
        p.path = "unfused"                                                                  # frozen
    m = net()
    m.use_rowblock = False
    q = m.forward_plan(1, 3, 64)
    m.use_rowblock = True
    assert q.path == "unfused" and q != p and m.forward_plan(1, 3, 64) is p


def test_one_definition_of_the_rowblock_limits():
    from gvfdiffusion_amd.ops import dit_ops
    for name in ("ROWBLOCK_C", "ROWBLOCK_ROWS", "ROWBLOCK_KPAD", "ROWBLOCK_MAX_HIDDEN", "ROWBLOCK_MAX_N3", "rowblock_supported", "rowblock_padded_rows"):
        assert getattr(dit_ops, name) is getattr(dit_plan, name)
    assert (dit_plan.ROWBLOCK_C, dit_plan.ROWBLOCK_ROWS, dit_plan.ROWBLOCK_KPAD, dit_plan.ROWBLOCK_MAX_HIDDEN, dit_plan.ROWBLOCK_MAX_N3) == (512, 48, 128, 2048, 1536)
    assert dit_plan.rowblock_padded_rows(8192) == 8208 and dit_plan.rowblock_padded_rows(144) == 144
    assert dit_plan.rowblock_supported(512, 8208, 2048) and not dit_plan.rowblock_supported(512, 8192, 2048) and not dit_plan.rowblock_supported(256, 48, 1024)
