"""Generates tests/golden/sparse_structure_golden.npz and sparse_structure_manifest.json by running the REFERENCE's
SparseStructureFlowModel, SparseStructureDecoder and guided Euler sampler (trellis/models/sparse_structure_flow.py,
sparse_structure_vae.py, trellis/pipelines/samplers/) on the CPU in fp32 with ATTN_BACKEND=naive and the package stubs of
make_slat_flow_golden.py.  Runs only where the reference checkout is (make_golden.py's REF); what it writes is data: inputs, outputs,
per-stage taps, a short sampler trajectory, the resulting coords, and the parameter names and shapes of the small and the released configs.
The weights are not stored: both sides take them from tests/sparse_structure_ref.py::make_weights.

The released configs (tests/sparse_structure_ref.py: FLOW_RELEASED, DEC_RELEASED) are written from memory of the public release -- the
pipeline JSON is not in the reference checkout -- and only their parameter names and shapes are recorded.

Usage:  python tests/golden/make_sparse_structure_golden.py"""
import importlib
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from make_slat_flow_golden import install_stubs  # noqa: E402
import conv3d_ref as C  # noqa: E402
import sparse_structure_ref as R  # noqa: E402


def load(model, seed):
    shapes = {k: tuple(v.shape) for k, v in model.named_parameters()}
    sd = {k: torch.from_numpy(v) for k, v in R.make_weights(shapes, seed).items()}
    for k, v in model.named_buffers():
        sd[k] = v
    model.load_state_dict(sd, strict=True)
    for name, p in model.named_parameters():
        assert float(p.abs().max()) > 0, f"{name} is all zero"
    return model.eval()


def tree(model):
    return {k: list(v.shape) for k, v in model.state_dict().items()}


def gen(out):
    flow = importlib.import_module("trellis.models.sparse_structure_flow")
    vae = importlib.import_module("trellis.models.sparse_structure_vae")
    smp = importlib.import_module("trellis.pipelines.samplers.flow_euler")
    manifest = {}

    # ---- the decoder -------------------------------------------------------------------------------------------------------------------
    dec = load(vae.SparseStructureDecoder(**R.DEC_SMALL), seed=4)
    taps = {}
    keep = lambda name: (lambda mod, args, output: taps.__setitem__(name, C.to_rows(output.detach())))
    dec.input_layer.register_forward_hook(keep("input"))
    for prefix, blocks in (("middle", dec.middle_block), ("block", dec.blocks)):
        for i, b in enumerate(blocks):
            b.register_forward_hook(keep(f"{prefix}{i}"))
            if hasattr(b, "conv1"):
                b.conv1.register_forward_hook(keep(f"{prefix}{i}_conv1"))
    z = R.decoder_input()
    with torch.no_grad():
        logits = dec(z)
    taps["logits"] = C.to_rows(logits)
    assert set(taps) == set(R.DEC_STAGES), sorted(taps)
    out["dec.z"], out["dec.logits"] = z.numpy(), logits.numpy()
    out["dec.coords"] = torch.argwhere(logits > 0)[:, [0, 2, 3, 4]].int().numpy()
    for k, v in taps.items():
        if k != "block2_conv1":                             # the file stays small: block2's output covers it
            out["dec.tap." + k] = v.numpy()
        print("decoder tap", k, tuple(v.shape), float(v.abs().mean()))
    print("decoder logits: mean", float(logits.mean()), "std", float(logits.std()), "occupied", out["dec.coords"].shape[0], "of", logits.numel())
    manifest["decoder_small"] = {"config": R.DEC_SMALL, "state_dict": tree(dec)}

    # ---- the flow models -----------------------------------------------------------------------------------------------------------------
    models = {}
    for name, cfg in R.FLOW_SMALL.items():
        model = models[name] = load(flow.SparseStructureFlowModel(**cfg), seed=3)
        taps = {}
        rows = lambda t: t.detach().reshape(-1, t.shape[-1]).clone()
        model.blocks[0].register_forward_pre_hook(lambda mod, args: taps.__setitem__("input", rows(args[0])))
        hooks = [b.register_forward_hook((lambda i: lambda mod, args, output: taps.__setitem__(f"block{i}", rows(output)))(i))
                 for i, b in enumerate(model.blocks)]
        hooks.append(model.out_layer.register_forward_hook(lambda mod, args, output: taps.__setitem__("out", rows(output))))
        x, t, cond = R.flow_inputs(name)
        with torch.no_grad():
            y = model(x, t, cond)
        for h in hooks:
            h.remove()
        out[f"flow.{name}.x"], out[f"flow.{name}.t"], out[f"flow.{name}.cond"], out[f"flow.{name}.y"] = x.numpy(), t.numpy(), cond.numpy(), y.numpy()
        for k, v in taps.items():
            if name == "p2" and k.startswith("block"):      # the file stays small: the second config keeps its first and last stage
                continue
            out[f"flow.{name}.tap.{k}"] = v.numpy()
            print("flow", name, "tap", k, tuple(v.shape), float(v.abs().mean()))
        manifest[f"flow_small_{name}"] = {"config": cfg, "state_dict": tree(model)}

    # ---- a short guided run through flow model, decoder and argwhere -----------------------------------------------------------------------
    x, _, cond = R.flow_inputs("p1")
    neg = torch.zeros_like(cond)
    ret = smp.FlowEulerGuidanceIntervalSampler(sigma_min=1e-5).sample(models["p1"], x, cond=cond, neg_cond=neg, verbose=False, **R.PIPE_PARAMS)
    with torch.no_grad():
        logits = dec(ret.samples)
    out["pipe.pred_x_t"], out["pipe.samples"] = torch.stack(ret.pred_x_t).numpy(), ret.samples.numpy()
    out["pipe.logits"] = logits.numpy()
    out["pipe.coords"] = torch.argwhere(logits > 0)[:, [0, 2, 3, 4]].int().numpy()
    print("pipeline: samples", float(ret.samples.abs().mean()), "occupied", out["pipe.coords"].shape[0], "of", logits.numel())

    # ---- the released configs' parameter trees, names and shapes only ------------------------------------------------------------------------
    with torch.device("meta"):
        manifest["flow_released"] = {"config": R.FLOW_RELEASED, "state_dict": tree(flow.SparseStructureFlowModel(**R.FLOW_RELEASED))}
        manifest["decoder_released"] = {"config": R.DEC_RELEASED, "state_dict": tree(vae.SparseStructureDecoder(**R.DEC_RELEASED))}
    with open(R.MANIFEST, "w") as f:
        json.dump(manifest, f, indent=0, sort_keys=True)
    for k, v in manifest.items():
        print("manifest", k, len(v["state_dict"]), "tensors,", sum(int(np.prod(s)) for s in v["state_dict"].values()) / 1e6, "M values")


if __name__ == "__main__":
    install_stubs()
    out = {}
    gen(out)
    np.savez_compressed(R.GOLD, **out)
    print(R.GOLD, os.path.getsize(R.GOLD), "bytes")
