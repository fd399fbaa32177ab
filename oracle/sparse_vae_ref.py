"""Torch restatement of the static-VAE backbone (SparseTransformerVAE) -- TEST INFRASTRUCTURE ONLY (see oracle/__init__.py).

Follows model/sparse_voxel_diffusion/sparse_transformer_vae.py: encode :158-182, decode :184-196; the block
sparse_transformer.py:165-191 (unmodulated branch: x + attn(LN(x)); x + mlp(LN(x)), LayerNorm eps 1e-6, no affine);
the absolute position embedder :73-112; the swin window partition sparse/attention/windowed_attn.py:20-60 (coords + shift,
// window, tokens grouped by (batch, wx, wy, wz)); the qkv channel layouts of sparse/attention/modules.py:150-162; softmax
attention inside a window with scale head_dim^-0.5 (flash_attn_varlen_qkvpacked_func, a third-party kernel -- restated
from its definition); tanh-GELU MLP :115-126.  Operates on (feats (T, C), coords (T, 4) = batch, x, y, z).
Pinned by tests/golden/sparse_vae_golden.npz (outputs of the reference classes imported in the build container).
attention_spans / multi_head_attention / block over spans / block_attn_rule / torso_spans restate the same computation over explicit
(batch, key rows, write rows) spans -- serialised windows, whose keys overlap, and all five attn_modes of block_attn_config
(sparse_transformer.py:11-25); the spans come from tests/sparse_ref.py, which is pinned by tests/golden/sparse_index_golden.npz.

precision "bf16" / "fp16" rounds where the HIP path rounds: every GEMM / attention operand (LayerNorm outputs, q k v, the
probabilities' numerators, the attention output, the GELU output) to that type, fp32 everywhere else."""
import torch
import torch.nn.functional as F


_LP = {"bf16": torch.bfloat16, "fp16": torch.float16}


def _r(x, precision):
    return x.to(_LP[precision]).to(torch.float32) if precision in _LP else x


def _lin(x, sd, name, precision):
    return F.linear(_r(x, precision), _r(sd[name + ".weight"], precision)) + sd[name + ".bias"]


def ape(xyz, channels):
    freq_dim = channels // 3 // 2
    freqs = 1.0 / (10000 ** (torch.arange(freq_dim, dtype=torch.float32) / freq_dim))
    out = torch.outer(xyz.reshape(-1).float(), freqs)
    e = torch.cat([torch.sin(out), torch.cos(out)], dim=-1).reshape(xyz.shape[0], -1)
    if e.shape[1] < channels:
        e = torch.cat([e, torch.zeros(xyz.shape[0], channels - e.shape[1])], dim=-1)
    return e


def window_ids(coords, window, shift):
    """One integer per token identifying its (batch, window): windowed_attn.py:34-47."""
    c = coords.long().clone()
    c[:, 1:] += shift
    n = [int(c[:, 1 + a].max()) // window + 1 for a in range(3)]
    w = c[:, 1:] // window
    return ((c[:, 0] * n[0] + w[:, 0]) * n[1] + w[:, 1]) * n[2] + w[:, 2]


def attention_groups(q, k, v, gid, precision):
    """q k v (T, H, d); softmax attention among the tokens sharing a group id."""
    out = torch.zeros_like(q)
    d = q.shape[-1]
    for g in torch.unique(gid):
        idx = torch.nonzero(gid == g).squeeze(1)
        qg, kg, vg = (t[idx].permute(1, 0, 2) for t in (q, k, v))                 # (H, n, d)
        s = (qg @ kg.transpose(-1, -2)) * d ** -0.5
        if precision in _LP:
            e = torch.exp(s - s.amax(dim=-1, keepdim=True))
            o = (_r(e, precision) @ vg) / e.sum(dim=-1, keepdim=True)
        else:
            o = torch.softmax(s, dim=-1) @ vg
        out[idx] = o.permute(1, 0, 2)
    return out


def attention_spans(q, k, v, spans, precision):
    """q (Tq, H, d), k v (Tk, H, d); spans: a list of (batch, key rows, write rows), index tensors into k / v and into q.  Softmax attention
    of each span's write rows over its key rows, in the order given; the output is taken at the write rows only (a serialised window
    gathers `window_size` key rows and writes back its valid span: sparse/attention/serialized_attn.py).  Rows no span writes stay zero; a
    row two spans write holds the later one's.  float64 inputs with precision "fp32": the reference; "bf16" / "fp16": attention_groups'
    rounding placement."""
    out = torch.zeros_like(q)
    d = q.shape[-1]
    for _, keys, writes in spans:
        qg = q[writes].permute(1, 0, 2)                                             # (H, n_w, d)
        kg, vg = k[keys].permute(1, 0, 2), v[keys].permute(1, 0, 2)                 # (H, n_k, d)
        s = (qg @ kg.transpose(-1, -2)) * d ** -0.5
        if precision in _LP:
            e = torch.exp(s - s.amax(dim=-1, keepdim=True))
            o = (_r(e, precision) @ vg) / e.sum(dim=-1, keepdim=True)
        else:
            o = torch.softmax(s, dim=-1) @ vg
        out[writes] = o.permute(1, 0, 2)
    return out


def _attend(q, k, v, groups, precision):
    """groups: a group id per token (attention_groups) or a list of spans (attention_spans)"""
    if isinstance(groups, (list, tuple)):
        return attention_spans(q, k, v, groups, precision)
    return attention_groups(q, k, v, groups, precision)


def _heads(rows, parts, heads, old_impl):
    """(T, parts * C) projection rows -> `parts` tensors (T, H, d): channels [head][part][c] (old_impl) or [part][head][c]
    (sparse/attention/modules.py:150-162)"""
    T = rows.shape[0]
    if old_impl:
        return rows.reshape(T, heads, parts, -1).unbind(dim=2)
    return rows.reshape(T, parts, heads, -1).unbind(dim=1)


def multi_head_attention(h, groups, sd, prefix, heads, precision, old_impl, qk_rms_norm=False, context=None, round_output=False):
    """SparseMultiHeadAttention (sparse/attention/modules.py:72-185) on rows h (T, C) -> (T, C): to_qkv (or, with a context (Tc, Cc), to_q
    and to_kv; the spans' key rows then index the context), the channel layout, optional QK-RMSNorm, attention per group / span, to_out.
    round_output: the closing projection's result is 16-bit too (torch.autocast's placement, which the module's enable_training() route
    follows; the inference route and the blocks keep it fp32)."""
    T, C = h.shape
    d = C // heads
    if context is None:
        q, k, v = _heads(_r(_lin(h, sd, prefix + ".to_qkv", precision), precision), 3, heads, old_impl)
    else:
        q = _r(_lin(h, sd, prefix + ".to_q", precision), precision).reshape(T, heads, d)
        k, v = _heads(_r(_lin(context, sd, prefix + ".to_kv", precision), precision), 2, heads, old_impl)
    if qk_rms_norm:   # SparseMultiHeadRMSNorm, trellis/modules/sparse/attention/modules.py:11-25: normalize * gamma * sqrt(d)
        q = _r(F.normalize(q, dim=-1) * sd[prefix + ".q_rms_norm.gamma"] * d ** 0.5, precision)
        k = _r(F.normalize(k, dim=-1) * sd[prefix + ".k_rms_norm.gamma"] * d ** 0.5, precision)
    a = _r(_attend(q, k, v, groups, precision).reshape(T, C), precision)
    y = _lin(a, sd, prefix + ".to_out", precision)
    return _r(y, precision) if round_output else y


def block(x, gid, sd, prefix, heads, precision, old_impl, qk_rms_norm=False):
    """gid: a group id per token, or a list of spans (attention_spans)."""
    T, C = x.shape
    h = _r(F.layer_norm(x, (C,), eps=1e-6), precision)
    x = x + multi_head_attention(h, gid, sd, prefix + ".attn", heads, precision, old_impl, qk_rms_norm)
    h = _r(F.layer_norm(x, (C,), eps=1e-6), precision)
    h = _r(F.gelu(_lin(h, sd, prefix + ".mlp.mlp.0", precision), approximate="tanh"), precision)
    return x + _lin(h, sd, prefix + ".mlp.mlp.2", precision)


def _torso(rows, coords, sd, cfg, first, stack, last, precision):
    C, heads, window = cfg["model_channels"], cfg["num_heads"], cfg["window_size"]
    assert cfg.get("attn_mode", "swin") == "swin" and cfg.get("pe_mode", "ape") == "ape"
    x = _lin(rows, sd, first, precision) + ape(coords[:, 1:], C)
    for i in range(cfg["num_blocks"]):
        gid = window_ids(coords, window, window // 2 * (i % 2))
        x = block(x, gid, sd, f"{stack}.{i}", heads, precision, cfg.get("use_old_attn_impl", True))
    if cfg.get("norm_output", False):
        x = F.layer_norm(x, (C,))
    return _lin(x, sd, last, precision)


ORDERS = ("Z_ORDER", "Z_ORDER_TRANSPOSED", "HILBERT", "HILBERT_TRANSPOSED")


def block_attn_rule(cfg, i):
    """Block i's attention plan, restated from block_attn_config (sparse_transformer.py:11-25): a dict with kind "full" | "windowed" |
    "serialized", window, shift (windowed: one integer for the three axes), shift_sequence, shift_window, order (a name of ORDERS)."""
    mode, w = cfg.get("attn_mode", "swin"), cfg["window_size"]
    if mode == "swin":
        return dict(kind="windowed", window=w, shift=w // 2 * (i % 2))
    if mode == "full":
        return dict(kind="full")
    rule = dict(kind="serialized", window=w, shift_sequence=0, shift_window=(0, 0, 0), order="Z_ORDER")
    if mode == "shift_window":
        rule["shift_window"] = (16 * (i % 2),) * 3
    elif mode == "shift_sequence":
        rule["shift_sequence"] = w // 2 * (i % 2)
    elif mode == "shift_order":
        rule["order"] = ORDERS[i % 4]
    else:
        raise ValueError(f"unknown attn_mode {mode}")
    return rule


def torso_spans(rows, coords, sd, cfg, first, stack, last, precision, make_spans):
    """_torso for all five attn_modes: block i attends over make_spans(block_attn_rule(cfg, i)), a list of spans (attention_spans) that
    the caller builds from the coordinates (tests/sparse_ref.py::spans_of_rule: the curve codes come from the C oracle)."""
    C, heads = cfg["model_channels"], cfg["num_heads"]
    assert cfg.get("pe_mode", "ape") == "ape"
    x = _lin(rows, sd, first, precision) + ape(coords[:, 1:], C).to(rows.dtype)
    for i in range(cfg["num_blocks"]):
        x = block(x, make_spans(block_attn_rule(cfg, i)), sd, f"{stack}.{i}", heads, precision, cfg.get("use_old_attn_impl", True))
    if cfg.get("norm_output", False):
        x = F.layer_norm(x, (C,))
    return _lin(x, sd, last, precision)


def encode_spans(sd, cfg, feats, coords, make_spans, precision="fp32"):
    return torso_spans(feats, coords, sd, cfg, "input_layer", "encoder", "to_latent", precision, make_spans).chunk(2, dim=-1)


def decode_spans(sd, cfg, z, coords, make_spans, precision="fp32"):
    return torso_spans(z, coords, sd, cfg, "from_latent", "decoder", "out_layer", precision, make_spans)


def encode(sd, cfg, feats, coords, precision="fp32"):
    """-> (mean, logvar), each (T, latent_channels)."""
    return _torso(feats, coords, sd, cfg, "input_layer", "encoder", "to_latent", precision).chunk(2, dim=-1)


def decode(sd, cfg, z, coords, precision="fp32"):
    return _torso(z, coords, sd, cfg, "from_latent", "decoder", "out_layer", precision)


def slat_decode_rows(sd, cfg, feats, coords, precision="fp32"):
    """TRELLIS SLatGaussianDecoder up to its output rows (trellis/models/structured_latent_vae/base.py:108-117,
    decoder_gs.py:117-121): input layer + APE, swin blocks ([q|k|v][head][c] layout, optional QK-RMSNorm), LayerNorm, out_layer."""
    C, heads, window = cfg["model_channels"], cfg["num_heads"], cfg["window_size"]
    x = _lin(feats, sd, "input_layer", precision) + ape(coords[:, 1:], C)
    for i in range(cfg["num_blocks"]):
        gid = window_ids(coords, window, window // 2 * (i % 2))
        x = block(x, gid, sd, f"blocks.{i}", heads, precision, False, cfg.get("qk_rms_norm", False))
    return _lin(F.layer_norm(x, (C,)), sd, "out_layer", precision)
