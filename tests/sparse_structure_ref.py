"""What the sparse-structure tests share: the small golden configs and the released ones, the weights (a NumPy Generator by parameter name
-- never stored), the inputs, and TorchOps: tests/slat_flow_ref.py's torch operator set with the dense convolution and the occupancy
read-out of gvfdiffusion_amd/trellis/models/structured_latent_flow.py::HipOps added.

The released configs are written from memory of the public TRELLIS-image-large release (the pipeline JSON is not part of the reference
checkout); nothing else is taken from them."""
import math
import os
import zlib

import numpy as np
import torch
import torch.nn.functional as F

import conv3d_ref as C
import slat_flow_ref as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sparse_structure_golden.npz")
MANIFEST = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sparse_structure_manifest.json")

_FLOW = dict(in_channels=8, model_channels=128, cond_channels=64, out_channels=8, num_blocks=2, num_heads=2, mlp_ratio=4, pe_mode="ape",
             use_fp16=False, share_mod=False, qk_rms_norm=True, qk_rms_norm_cross=False)
FLOW_SMALL = {"p1": dict(_FLOW, resolution=4, patch_size=1), "p2": dict(_FLOW, resolution=8, patch_size=2)}
FLOW_RELEASED = dict(resolution=16, in_channels=8, model_channels=1024, cond_channels=1024, out_channels=8, num_blocks=24, num_heads=16,
                     mlp_ratio=4, patch_size=1, pe_mode="ape", use_fp16=True, share_mod=False, qk_rms_norm=True, qk_rms_norm_cross=False)
DEC_SMALL = dict(out_channels=1, latent_channels=8, num_res_blocks=1, channels=[64, 32], num_res_blocks_middle=1, norm_type="layer",
                 use_fp16=False)
DEC_RELEASED = dict(out_channels=1, latent_channels=8, num_res_blocks=2, channels=[512, 128, 32], num_res_blocks_middle=2, norm_type="layer",
                    use_fp16=True)
COND_TOKENS = 37
BATCH = 2
# the out layer's bias: a little over two standard deviations of the small decoder's logits below zero, so that a few per cent of the cells are occupied
# and few logits sit near zero (tests/test_sparse_structure_host.py asserts how few)
LOGIT_BIAS = -1.1
PIPE_PARAMS = dict(steps=3, cfg_strength=3.0, cfg_interval=(0.5, 1.0), rescale_t=3.0)
DEC_STAGES = ["input", "middle0_conv1", "middle0", "block0_conv1", "block0", "block1", "block2_conv1", "block2", "logits"]
FLOW_STAGES = ["input", "block0_self", "block0_cross", "block0", "block1_self", "block1_cross", "block1", "out"]


def build_flow(cfg, device=None):
    from gvfdiffusion_amd.trellis.models import SparseStructureFlowModel
    if device is None:
        return SparseStructureFlowModel(**cfg).eval()
    with torch.device(device):
        return SparseStructureFlowModel(**cfg).eval()


def build_decoder(cfg, device=None):
    from gvfdiffusion_amd.trellis.models import SparseStructureDecoder
    if device is None:
        return SparseStructureDecoder(**cfg).eval()
    with torch.device(device):
        return SparseStructureDecoder(**cfg).eval()


def make_weights(shapes, seed):
    """name -> fp32 array for every PARAMETER in `shapes` (name -> shape): a Generator per name (seed, crc32(name)), so the values do not
    depend on the order of the state dict.  Every tensor the models zero-initialise (conv2, adaLN_modulation, out_layer) is non-zero."""
    out = {}
    for name, shape in shapes.items():
        g = np.random.default_rng([seed, zlib.crc32(name.encode())])
        leaf = name.rsplit(".", 1)[-1]
        if name == "out_layer.2.bias":
            w = np.full(shape, LOGIT_BIAS)
        elif leaf == "gamma" or (leaf == "weight" and len(shape) == 1):
            w = 1.0 + 0.1 * g.standard_normal(shape)
        elif leaf == "bias":
            w = 0.1 * g.standard_normal(shape)
        elif len(shape) == 5:                                   # conv weight [out, in, 3, 3, 3] (or 1, 1, 1)
            w = g.standard_normal(shape) / math.sqrt(shape[1] * shape[2] * shape[3] * shape[4])
        elif "adaLN_modulation" in name:
            w = 0.5 * g.standard_normal(shape) / math.sqrt(shape[1])
        else:
            w = g.standard_normal(shape) / math.sqrt(shape[1])
        out[name] = w.astype(np.float32)
    return out


def param_shapes(model):
    return {k: tuple(v.shape) for k, v in model.named_parameters()}


def load_weights(model, seed):
    """Seeded weights into every parameter, strictly; the buffers (pos_emb) stay the model's own."""
    sd = {k: torch.from_numpy(v) for k, v in make_weights(param_shapes(model), seed).items()}
    for k, v in model.named_buffers():
        sd[k] = v
    model.load_state_dict(sd, strict=True)
    return model


def flow_inputs(name, seed=5):
    """(x fp32 (2, 8, R, R, R), t fp32 (2,), cond fp32 (2, 37, 64)) of the small flow config `name`."""
    cfg = FLOW_SMALL[name]
    g = torch.Generator().manual_seed(seed + cfg["resolution"])
    R_ = cfg["resolution"]
    x = torch.randn((BATCH, cfg["in_channels"], R_, R_, R_), generator=g)
    cond = torch.randn((BATCH, COND_TOKENS, cfg["cond_channels"]), generator=g)
    return x, torch.tensor([700.0, 130.0]), cond


def decoder_input(seed=6):
    """z fp32 (2, 8, 4, 4, 4)."""
    return torch.randn((BATCH, DEC_SMALL["latent_channels"], 4, 4, 4), generator=torch.Generator().manual_seed(seed))


class TorchOps(R.TorchOps):
    def dense_conv3(self, a16, grid, conv, addend=None, store="rows"):
        x = C.to_dense(a16[:, :conv.in_channels].to(self.acc), grid)
        y = C.to_rows(F.conv3d(x, self._op(conv.weight), self._a(conv.bias), padding=1))
        if store == "shuffle2":
            y = C.pixel_shuffle2(y, grid)
        return y if addend is None else y + addend.to(self.acc)

    @staticmethod
    def occupancy(logits, grid):
        B, X, Y, Z = grid
        return torch.argwhere(logits.reshape(B, 1, X, Y, Z) > 0)[:, [0, 2, 3, 4]].int()


def run_decoder(dec, z, ops, taps=None):
    """-> logit rows (B 8^3, 1) through `ops`."""
    B, _, X, Y, Z = z.shape
    return dec.forward_rows(C.to_rows(z), (B, X, Y, Z), ops, taps)[0]


def pipeline_logits(flow, dec, ops, dtype=torch.float32):
    """The golden's short guided run (flow config "p1", PIPE_PARAMS, the noise and tokens of flow_inputs) through `ops`, then the decoder
    -> (latent (2, 8, 4, 4, 4), logit rows (2 8^3, 1))."""
    from gvfdiffusion_amd.trellis.pipelines import samplers as smp
    x, _, cond = flow_inputs("p1")
    x, cond = x.to(dtype), cond.to(dtype)
    z = smp.FlowEulerGuidanceIntervalSampler(sigma_min=1e-5).sample(flow, x, cond=cond, neg_cond=torch.zeros_like(cond), verbose=False, ops=ops,
                                                                    **PIPE_PARAMS).samples
    return z, run_decoder(dec, z, ops)
