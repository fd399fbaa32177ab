"""Generates tests/golden/slat_flow_golden.npz and slat_flow_manifest.json by running the REFERENCE's SLatFlowModel and Euler samplers
(trellis/models/structured_latent_flow.py, trellis/pipelines/samplers/) on the CPU in fp32.  Runs only where the reference checkout is
(make_golden.py's REF); what it writes is data: coordinates, inputs, t, condition, outputs, per-stage taps, sampler trajectories and the
released config's parameter names and shapes.  The weights are not stored: both sides take them from tests/slat_flow_ref.py::make_weights.

Stand-ins for what the reference imports and this image lacks (module level, throw-away, nothing shipped):
  spconv.pytorch.SparseConvTensor   a plain record of the fields trellis/modules/sparse/basic.py touches
  spconv.pytorch.SubMConv3d         weight [out, k, k, k, in] + bias; forward = the operator's definition in its dense form:
                                    F.conv3d(densified grid, weight.permute(0, 4, 1, 2, 3), bias, padding = k // 2) read back at the sites
  flash_attn                        the three varlen entry points as softmax attention in torch
  easydict                          a dict subclass;  tqdm: a pass-through if missing

Usage:  python tests/golden/make_slat_flow_golden.py"""
import importlib
import json
import os
import sys

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from make_golden import REF, _stub  # noqa: E402
import slat_flow_ref as R  # noqa: E402


def install_stubs():
    os.environ["ATTN_BACKEND"] = "naive"
    os.environ["SPARSE_ATTN_BACKEND"] = "flash_attn"
    os.environ["SPARSE_BACKEND"] = "spconv"

    class SparseConvTensor:
        def __init__(self, features, indices, spatial_shape, batch_size, grid=None, voxel_num=None, indice_dict=None, benchmark=False):
            self._features, self.indices, self.spatial_shape, self.batch_size = features, indices, spatial_shape, batch_size
            self.grid, self.voxel_num, self.indice_dict, self.benchmark = grid, voxel_num, indice_dict, benchmark
            self.benchmark_record = self.thrust_allocator = self._timer = self.force_algo = self.int8_scale = None

        @property
        def features(self):
            return self._features

    class SubMConv3d(nn.Module):
        def __init__(self, in_channels, out_channels, kernel_size, dilation=1, bias=True, indice_key=None, algo=None):
            super().__init__()
            assert dilation == 1
            self.in_channels, self.out_channels, self.k = in_channels, out_channels, kernel_size
            self.weight = nn.Parameter(torch.zeros((out_channels, kernel_size, kernel_size, kernel_size, in_channels)))
            self.bias = nn.Parameter(torch.zeros(out_channels)) if bias else None

        def forward(self, data):
            c = data.indices.long()
            B = int(c[:, 0].max()) + 1
            ext = (c[:, 1:].max(0).values + 1).tolist()
            grid = torch.zeros((B, self.in_channels, *ext), dtype=data.features.dtype)
            grid[c[:, 0], :, c[:, 1], c[:, 2], c[:, 3]] = data.features
            y = torch.nn.functional.conv3d(grid, self.weight.permute(0, 4, 1, 2, 3), self.bias, padding=self.k // 2)
            return SparseConvTensor(y[c[:, 0], :, c[:, 1], c[:, 2], c[:, 3]], data.indices, data.spatial_shape, data.batch_size)

    def attn(q, k, v):                                   # (n, H, d), (m, H, d) -> (n, H, d)
        s = torch.einsum("nhd,mhd->hnm", q, k) * q.shape[-1] ** -0.5
        return torch.einsum("hnm,mhd->nhd", torch.softmax(s, dim=-1), v)

    def varlen(q, k, v, cu_q, cu_k, max_q=None, max_k=None, **kw):
        out = torch.empty_like(q)
        for a, b, c, d in zip(cu_q[:-1].tolist(), cu_q[1:].tolist(), cu_k[:-1].tolist(), cu_k[1:].tolist()):
            out[a:b] = attn(q[a:b], k[c:d], v[c:d])
        return out

    spc = _stub("spconv")
    spc.pytorch = _stub("spconv.pytorch", SparseConvTensor=SparseConvTensor, SubMConv3d=SubMConv3d)
    _stub("flash_attn",
          flash_attn_varlen_qkvpacked_func=lambda qkv, cu, mx, **kw: varlen(*qkv.unbind(dim=1), cu, cu),
          flash_attn_varlen_kvpacked_func=lambda q, kv, cu_q, cu_k, mq, mk, **kw: varlen(q, *kv.unbind(dim=1), cu_q, cu_k),
          flash_attn_varlen_func=lambda q, k, v, cu_q, cu_k, mq, mk, **kw: varlen(q, k, v, cu_q, cu_k))

    class EasyDict(dict):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            self.__dict__ = self
    _stub("easydict", EasyDict=EasyDict)
    try:
        import tqdm  # noqa: F401
    except ImportError:
        _stub("tqdm", tqdm=lambda it, **kw: it)
    # the trellis package is entered through path-only package stubs, so that its pipelines / renderers are never imported
    for name in ("trellis", "trellis.models", "trellis.pipelines"):
        pkg = _stub(name)
        pkg.__path__ = [f"{REF}/" + name.replace(".", "/")]


def gen_model(out):
    flow = importlib.import_module("trellis.models.structured_latent_flow")
    tsp = importlib.import_module("trellis.modules.sparse")
    torch.manual_seed(0)
    model = flow.SLatFlowModel(**{k: v for k, v in R.SMALL.items()}).eval()
    weights = R.make_weights(R.SMALL, seed=3)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in weights.items()}, strict=True)
    for name, p in model.named_parameters():
        assert float(p.abs().max()) > 0, f"{name} is all zero"
    coords, feats, t, cond = R.golden_inputs()
    taps = {}

    def keep(name):
        def hook(mod, args, output):
            taps[name] = output.feats.detach().clone()
        return hook

    model.input_layer.register_forward_hook(keep("input"))
    for i, b in enumerate(model.input_blocks):
        b.register_forward_hook(keep(f"in{i}"))
        b.conv1.register_forward_hook(keep(f"in{i}_conv1"))
    for i, b in enumerate(model.blocks):
        b.register_forward_hook(keep(f"block{i}"))
    for i, b in enumerate(model.out_blocks):
        b.register_forward_hook(keep(f"out{i}"))
    with torch.no_grad():
        y = model(tsp.SparseTensor(feats, coords), t, cond)
    out["cfg_json"] = np.frombuffer(json.dumps(R.SMALL).encode(), dtype=np.uint8)
    out["coords"], out["feats"], out["t"], out["cond"], out["out"] = coords.numpy(), feats.numpy(), t.numpy(), cond.numpy(), y.feats.numpy()
    for k, v in taps.items():
        out["tap." + k] = v.numpy()
        print("tap", k, tuple(v.shape), float(v.abs().mean()))
    print("slat_flow out", tuple(y.feats.shape), float(y.feats.abs().mean()))
    # the released config's parameter tree, names and shapes only
    with torch.device("meta"):
        big = flow.SLatFlowModel(**{k: v for k, v in R.RELEASED.items()})
    manifest = {k: list(v.shape) for k, v in big.state_dict().items()}
    with open(R.MANIFEST, "w") as f:
        json.dump({"config": R.RELEASED, "state_dict": manifest}, f, indent=0, sort_keys=True)
    print("manifest", len(manifest), "tensors,", sum(int(np.prod(s)) for s in manifest.values()) / 1e6, "M parameters")


def gen_samplers(out):
    smp = importlib.import_module("trellis.pipelines.samplers.flow_euler")
    noise, cond, neg = R.sampler_inputs()
    for name, case in R.SAMPLER_CASES.items():
        s = getattr(smp, case["cls"])(sigma_min=1e-5)
        kw = dict(case["kw"], verbose=False)
        if case.get("neg"):
            kw["neg_cond"] = neg
        ret = s.sample(R.standin_model, noise, cond, **kw)
        out[f"sampler.{name}.samples"] = ret.samples.numpy()
        out[f"sampler.{name}.pred_x_t"] = torch.stack(ret.pred_x_t).numpy()
        out[f"sampler.{name}.pred_x_0"] = torch.stack(ret.pred_x_0).numpy()
        print("sampler", name, float(ret.samples.abs().mean()))


if __name__ == "__main__":
    install_stubs()
    out = {}
    gen_model(out)
    gen_samplers(out)
    np.savez_compressed(R.GOLD, **out)
    print(R.GOLD, os.path.getsize(R.GOLD), "bytes")
