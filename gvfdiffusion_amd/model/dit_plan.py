"""Which launches one DiT forward makes, decided once in plain host code: no device, no library, no tensors (DESIGN.md section 3.2,
"which launches a forward makes").  model/dit.py asks `plan_forward` and runs what the plan says; tests/test_dit_plan_host.py pins the
decision table on the CPU, tests/test_dit_plan_gpu.py checks that the plan is what runs."""
import functools
import os
from dataclasses import dataclass, field
from typing import Mapping, NamedTuple, Optional, Tuple

# the row-block launch (csrc/rowblock.hip): model_channels, rows per block, K padding of its first projection, widest MLP, widest third projection
ROWBLOCK_C, ROWBLOCK_ROWS, ROWBLOCK_KPAD, ROWBLOCK_MAX_HIDDEN, ROWBLOCK_MAX_N3 = 512, 48, 128, 2048, 1536


def rowblock_supported(C: int, rows_per_group: int, hidden: int) -> bool:
    """The row-block kernel covers model_channels 512, 48-row blocks that do not straddle samples (callers pad a sample's rows to a
    multiple of 48: rowblock_padded_rows), an MLP of <= 2048 hidden units."""
    return C == ROWBLOCK_C and rows_per_group % ROWBLOCK_ROWS == 0 and hidden % ROWBLOCK_C == 0 and 0 < hidden <= ROWBLOCK_MAX_HIDDEN


def rowblock_padded_rows(rows: int) -> int:
    """Rows of a sample rounded up to whole 48-row blocks."""
    return (rows + ROWBLOCK_ROWS - 1) // ROWBLOCK_ROWS * ROWBLOCK_ROWS


class DiTSwitches(NamedTuple):
    """The path switches of a forward.  DiT keeps them as writable attributes (use_rowblock, rowblock_tiled_kv, rowblock_temporal,
    weight_prefetch, fuse_layernorm, modulation_table); every forward reads them into one of these."""
    rowblock: bool = True          # one launch per sub-layer boundary (csrc/rowblock.hip) where the shapes allow it
    tiled_kv: bool = True          # to_qkv's row-block launch writes the spatial attention's K / V^T tiles itself
    temporal_fused: bool = True    # the temporal self attention runs inside the row-block launch (T | 48)
    prefetch: bool = True          # an attention launch touches the packed weights of the row-block launch behind it
    fuse_ln: int = 0               # LayerNorm folded into the unfused path's GEMMs: 0 off, 1 every projection, 2 only N <= 512
    modtable: bool = True          # precompute_modulation builds its table

    @classmethod
    def from_env(cls, env=None):
        env = os.environ if env is None else env
        on = lambda name: int(env.get(name, "1")) != 0
        return cls(rowblock=on("GVF_DIT_ROWBLOCK"), tiled_kv=on("GVF_DIT_TILED_KV"), temporal_fused=on("GVF_DIT_TEMPORAL_FUSED"),
                   prefetch=on("GVF_DIT_PREFETCH"), fuse_ln=int(env.get("GVF_DIT_FUSE_LN", "0")), modtable=on("GVF_DIT_MODTABLE"))


class DiTGeometry(NamedTuple):
    C: int
    H: int
    head_dim: int
    Cin: int
    Cout: int
    hidden: int
    fdim: int
    n_blocks: int
    no_temporal_attn: bool

    @property
    def small_f32(self) -> bool:
        """input_layer and the final layer run in fp32 straight on the stream (csrc/elem.hip)"""
        return self.C <= 512 and self.C % 4 == 0 and self.Cin <= 24 and self.Cout <= 32

    @property
    def mod_f32(self) -> bool:
        """timestep embedder and adaLN projections as two fp32 launches; otherwise three 16-bit GEMMs"""
        return self.fdim % 4 == 0 and self.fdim <= 1024 and self.C % 4 == 0 and self.C <= 1024


class FrameViews(NamedTuple):
    """Per-frame views of the row buffers for the attentions of the row-block path: (outer, inner) problem counts, element strides
    (outer, inner, row) of a C-wide and a 3C-wide buffer, key-set strides (outer, inner), and the (sample, frame) view of the static
    attention, whose key set is per sample."""
    n: Tuple[int, int]
    c: Tuple[int, int, int]
    c3: Tuple[int, int, int]
    kv: Tuple[int, int]
    static: Tuple[int, int, int]


@dataclass(frozen=True)
class ForwardPlan:
    path: str                      # "rowblock" | "unfused"
    small_f32: bool
    mod_f32: bool
    TN: int                        # rows of one sample
    TNp: int                       # ... in the row buffers: whole 48-row blocks on the row-block path, TN otherwise
    padded: bool
    M: int                         # rows of every row buffer
    tiled_kv: bool
    temporal_fused: bool
    prefetch: bool
    fuse_ln: bool
    fuse_max_n: int                # widest projection that takes the folded LayerNorm
    strided_attention: bool        # csrc/attn.hip on row-major q / k / v instead of the tiled K / V cache
    frames: Optional[FrameViews]   # row-block path only
    streams: Tuple[str, ...]       # packed weight streams one block needs
    spatial_prefetch_stream: Optional[str]
    attention_workgroups: int      # tiled-attention workgroups of one forward (see DiT.count_attention_fallbacks)
    # dit_ops function -> calls per forward, the modulation apart (a hit in precompute_modulation's table removes its launches)
    launches: Mapping[str, int] = field(compare=False)
    modulation_launches: Mapping[str, int] = field(compare=False)


LAUNCH_NAMES = ("rowblock_fused", "attention_tiled", "attention", "attention_pack_kv", "gemm", "gemm_resid_stats", "gemm_ln_bf16",
                "layernorm_modulate", "cast_pad", "input_layer_f32", "final_layer_f32")


@functools.lru_cache(maxsize=256)
def plan_forward(g: DiTGeometry, sw: DiTSwitches, B: int, T: int, N: int) -> ForwardPlan:
    C, nb, temporal = g.C, g.n_blocks, not g.no_temporal_attn
    TN = T * N
    small_f32 = g.small_f32
    # the row-block launches work on whole 48-row blocks of one sample: a sample whose T * N is not a multiple of 48 (T = 16, 32 at
    # N = 512) gets its rows padded (needs whole 64-key tiles per frame for the attention's strided views: N % 64 == 0)
    TNp = rowblock_padded_rows(TN)
    rowblock = sw.rowblock and g.head_dim == 32 and small_f32 and g.Cin % 4 == 0 and g.Cin <= 16 and rowblock_supported(C, TNp, g.hidden) \
        and (TNp == TN or (N % 64 == 0 and sw.tiled_kv))
    if not rowblock:
        TNp = TN
    tiled_kv = rowblock and N % 64 == 0 and sw.tiled_kv
    # (a padded sample's padding rows are exactly the phantom tokens of its last block: ceil(N / (48 / T)) * 48 == TNp)
    temporal_fused = rowblock and sw.temporal_fused and temporal and ROWBLOCK_ROWS % T == 0
    padded = TNp != TN
    fuse_ln = not rowblock and sw.fuse_ln != 0 and TN % 128 == 0 and C % 128 == 0 and C <= 1024
    fuse_max_n = 1 << 30 if sw.fuse_ln == 1 else 512
    strided = g.head_dim != 32

    n = dict.fromkeys(LAUNCH_NAMES, 0)
    if rowblock:
        # per-frame views.  Padded: outer = sample (stride TNp rows), inner = frame (N rows), key set of (b, f) = b T + f; otherwise the
        # frames of all samples are one uniform run (the launch geometry the kernels were tuned on)
        if padded:
            frames = FrameViews(n=(B, T), c=(TNp * C, N * C, C), c3=(TNp * 3 * C, N * 3 * C, 3 * C), kv=(T, 1), static=(TNp * C, N * C, C))
        else:
            frames = FrameViews(n=(B * T, 1), c=(N * C, 0, C), c3=(N * 3 * C, 0, 3 * C), kv=(1, 0), static=(TNp * C, N * C, C))
        streams = ("s23", "s4", "s5") if temporal_fused else ("s2", "s4", "s5") if not temporal else ("s2", "s3", "s4", "s5")
        spatial_prefetch = streams[0] if tiled_kv else None
        n["rowblock_fused"] = 1 + nb * len(streams)
        n["attention_tiled"] = 3 * nb
        n["attention_pack_kv"] = 0 if tiled_kv else nb
        n["attention"] = nb if temporal and not temporal_fused else 0
        n["final_layer_f32"] = 1
    else:
        frames, streams, spatial_prefetch = None, (), None
        # every projection that follows a LayerNorm, in launch order; the fp32 input layer writes no row statistics, so after it the
        # first projection normalises with the LayerNorm launch whatever the switch says
        widths = ([3 * C] * (2 if temporal else 1) + [C, C, g.hidden]) * nb + ([] if small_f32 else [g.Cout])
        folded = sum(1 for j, w in enumerate(widths) if fuse_ln and (j > 0 or not small_f32) and w <= fuse_max_n)
        resid = (4 + temporal) * nb + (0 if small_f32 else 1)
        n["gemm_ln_bf16"] = folded
        n["layernorm_modulate"] = len(widths) - folded
        n["gemm_resid_stats"] = resid if fuse_ln else 0
        n["gemm"] = len(widths) - folded + (0 if fuse_ln else resid)
        n["input_layer_f32" if small_f32 else "cast_pad"] = 1
        n["final_layer_f32"] = 1 if small_f32 else 0
        n["attention"] = (3 + temporal) * nb if strided else temporal * nb
        n["attention_tiled"] = 0 if strided else 3 * nb
        n["attention_pack_kv"] = 0 if strided else nb
    mod = {"timestep_embed_f32": 1, "modulation_f32": 1} if g.mod_f32 else {"cast_pad": 3, "gemm": 3}
    return ForwardPlan(path="rowblock" if rowblock else "unfused", small_f32=small_f32, mod_f32=g.mod_f32, TN=TN, TNp=TNp, padded=padded,
                       M=B * TNp, tiled_kv=tiled_kv, temporal_fused=temporal_fused, prefetch=rowblock and sw.prefetch, fuse_ln=fuse_ln,
                       fuse_max_n=fuse_max_n, strided_attention=strided, frames=frames, streams=streams,
                       spatial_prefetch_stream=spatial_prefetch, attention_workgroups=nb * 3 * B * T * g.H * ((N + 255) // 256),
                       launches=n, modulation_launches=mod)
