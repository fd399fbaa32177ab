"""Host side of the sparse-convolution family and the structured-latent flow model (no GPU): the C ABI of include/gvf_spconv.h refuses
every malformed argument before a launch, the operators refuse CPU tensors, the modules construct (and refuse) as documented, the released
config has exactly the reference's parameter tree, the route through the torch operator set reproduces the reference-pinned golden, and
the three Euler samplers reproduce the reference's trajectories on a closed-form stand-in model."""
import ctypes
import json

import numpy as np
import pytest
import torch

import slat_flow_ref as R
from gvfdiffusion_amd import _lib, sparse as sp
from gvfdiffusion_amd.ops import spconv
from gvfdiffusion_amd.trellis import models as tm
from gvfdiffusion_amd.trellis.pipelines import samplers as smp

EINVAL, ENOSPC = _lib.GVF_EINVAL, _lib.GVF_ENOSPC
A = 0x10000                  # a fake 256-byte aligned device address: every call below must return before it would be touched
P = ctypes.c_void_p


def test_exports_and_size_queries():
    l = _lib.lib()
    for name in ("gvf_spconv_map_workspace_bytes", "gvf_spconv_neighbor_map", "gvf_spconv_packed_bytes", "gvf_spconv_pack", "gvf_spconv3",
                 "gvf_ln_act_rows"):
        assert name in _lib.SIGNATURES and hasattr(l, name)
    assert spconv.packed_bytes(128, 64) == 128 * 64 * 27 * 2
    assert spconv.packed_bytes(2048, 2048) == 2048 * 2048 * 27 * 2
    assert spconv.map_workspace_bytes(1) == 64 * 12 and spconv.map_workspace_bytes(1192) == 4096 * 12
    assert spconv.map_workspace_bytes(2048) == 4096 * 12 and spconv.map_workspace_bytes(2049) == 8192 * 12
    out = ctypes.c_size_t(0)
    for T in (0, -3, (1 << 31) // 27 + 1):
        assert l.gvf_spconv_map_workspace_bytes(T, ctypes.byref(out)) == EINVAL
    assert l.gvf_spconv_map_workspace_bytes(5, None) == EINVAL
    for cout, cin in ((0, 64), (64, 0), (32, 64), (96, 64), (64, 100), (2112, 64), (64, 4096), (-64, 64)):
        assert l.gvf_spconv_packed_bytes(cout, cin, ctypes.byref(out)) == EINVAL
    assert l.gvf_spconv_packed_bytes(64, 64, None) == EINVAL


def test_neighbor_map_and_pack_refuse_bad_arguments():
    l = _lib.lib()
    ws = 4096 * 12
    ok = dict(coords=A, T=1192, nbr=A, ws=A, nb=ws)
    call = lambda **kw: (lambda a: l.gvf_spconv_neighbor_map(P(a["coords"]), a["T"], P(a["nbr"]), P(a["ws"]), a["nb"], None))(dict(ok, **kw))
    for kw in (dict(coords=0), dict(nbr=0), dict(ws=0), dict(T=0), dict(T=-1), dict(T=(1 << 31) // 27 + 1), dict(coords=A + 4), dict(coords=A + 8),
               dict(nbr=A + 2), dict(ws=A + 128), dict(ws=A + 16)):
        assert call(**kw) == EINVAL, kw
    assert call(nb=ws - 1) == ENOSPC and call(nb=0) == ENOSPC
    okp = dict(w=A, cout=64, cin=128, dtype=0, out=A, nb=64 * 128 * 54)
    pack = lambda **kw: (lambda a: l.gvf_spconv_pack(P(a["w"]), a["cout"], a["cin"], a["dtype"], P(a["out"]), a["nb"], None))(dict(okp, **kw))
    for kw in (dict(w=0), dict(out=0), dict(dtype=2), dict(dtype=-1), dict(dtype=7), dict(cout=96), dict(cout=0), dict(cin=32), dict(cin=2112),
               dict(w=A + 2), dict(out=A + 8)):
        assert pack(**kw) == EINVAL, kw
    assert pack(nb=64 * 128 * 54 - 2) == ENOSPC


def test_conv_refuses_bad_arguments():
    l = _lib.lib()
    ok = dict(x=A, ld=64, nbr=A, w=A, bias=A, add=A, out=A, f32=1, T=100, cin=64, cout=128, dtype=1)

    def call(**kw):
        a = dict(ok, **kw)
        return l.gvf_spconv3(P(a["x"]), a["ld"], P(a["nbr"]), P(a["w"]), P(a["bias"]), P(a["add"]), P(a["out"]), a["f32"], a["T"], a["cin"], a["cout"],
                             a["dtype"], None)
    bad = [dict(x=0), dict(nbr=0), dict(w=0), dict(out=0), dict(dtype=2), dict(dtype=-1), dict(cin=0), dict(cin=32), dict(cin=96), dict(cin=2112),
           dict(cout=0), dict(cout=100), dict(cout=4096), dict(T=0), dict(T=-5), dict(T=(1 << 31) // 27 + 1), dict(ld=56), dict(ld=63),
           dict(cin=128, ld=64), dict(ld=68), dict(x=A + 8), dict(x=A + 2), dict(nbr=A + 2), dict(w=A + 8), dict(out=A + 8), dict(out=A + 4, f32=0),
           dict(bias=A + 4), dict(add=A + 8)]
    for kw in bad:
        assert call(**kw) == EINVAL, kw


def test_ln_act_refuses_bad_arguments():
    l = _lib.lib()
    ok = dict(dtype=0, x=A, out=A, rows=10, C=128, eps=1e-6, w=A, b=A, sh=A, sc=A, act=1)

    def call(**kw):
        a = dict(ok, **kw)
        return l.gvf_ln_act_rows(a["dtype"], P(a["x"]), P(a["out"]), a["rows"], a["C"], a["eps"], P(a["w"]), P(a["b"]), P(a["sh"]), P(a["sc"]),
                                 a["act"], None)
    bad = [dict(x=0), dict(out=0), dict(dtype=2), dict(dtype=-1), dict(rows=0), dict(rows=-1), dict(C=0), dict(C=2), dict(C=6), dict(C=2052),
           dict(C=4096), dict(eps=-1.0), dict(eps=float("nan")), dict(w=0), dict(b=0), dict(sh=0), dict(sc=0), dict(act=2), dict(act=-1),
           dict(x=A + 8), dict(out=A + 4), dict(w=A + 4), dict(b=A + 8), dict(sh=A + 4), dict(sc=A + 12)]
    for kw in bad:
        assert call(**kw) == EINVAL, kw


def test_operators_refuse_cpu_tensors():
    coords = torch.zeros((4, 4), dtype=torch.int32)
    with pytest.raises(_lib.GvfError):
        spconv.build_neighbor_map(coords)
    with pytest.raises(_lib.GvfError):
        spconv.pack_weight(torch.zeros((64, 3, 3, 3, 64)), torch.bfloat16)
    with pytest.raises(_lib.GvfError):
        spconv.conv3(torch.zeros((4, 64), dtype=torch.bfloat16), torch.zeros((4, 27), dtype=torch.int32), torch.zeros(64 * 64 * 54, dtype=torch.uint8), 64)
    with pytest.raises(_lib.GvfError):
        spconv.ln_act(torch.zeros((4, 64)))
    x = sp.SparseTensor(torch.zeros((4, 64)), coords + torch.arange(4, dtype=torch.int32)[:, None] * torch.tensor([0, 1, 0, 0], dtype=torch.int32))
    with pytest.raises(_lib.GvfError):
        sp.SparseConv3d(64, 64, 3)(x)


def test_sparse_conv3d_construction_and_refusals():
    c = sp.SparseConv3d(64, 128, 3)
    assert set(c.state_dict()) == {"conv.weight", "conv.bias"}
    assert tuple(c.conv.weight.shape) == (128, 3, 3, 3, 64) and tuple(c.conv.bias.shape) == (128,)
    assert set(sp.SparseConv3d(64, 128, 3, bias=False).state_dict()) == {"conv.weight"}
    assert tuple(sp.SparseConv3d(8, 16, 1).conv.weight.shape) == (16, 1, 1, 1, 8)
    for kw in (dict(stride=2), dict(padding=1), dict(dilation=2), dict(kernel_size=5), dict(kernel_size=2), dict(stride=(1, 2, 1)), dict(padding=0)):
        with pytest.raises(NotImplementedError, match="not built|is built"):
            sp.SparseConv3d(64, 64, **dict(dict(kernel_size=3), **kw))
    with pytest.raises(NotImplementedError, match="SparseInverseConv3d is not built"):
        sp.SparseInverseConv3d(64, 64, 3)
    from gvfdiffusion_amd.model.sparse_voxel_diffusion.sparse_transformer import SparseTransformerBlock
    with pytest.raises(NotImplementedError):                      # the unmodulated block's refusal is unchanged: the new block is a new class
        SparseTransformerBlock(128, 2, modulated=True)
    for kw in (dict(pe_mode="rope"), dict(share_mod=True)):
        with pytest.raises(NotImplementedError, match="not built"):
            tm.SLatFlowModel(**dict(R.SMALL, **kw))
    with pytest.raises(NotImplementedError, match="not built"):
        tm.ModulatedSparseTransformerCrossBlock(128, 64, 2, share_mod=True)
    with pytest.raises(NotImplementedError, match="not built"):
        tm.ModulatedSparseTransformerCrossBlock(128, 64, 2, use_rope=True)


def test_released_config_has_the_reference_parameter_tree():
    want = json.load(open(R.MANIFEST))
    assert want["config"] == R.RELEASED
    got = {k: list(v.shape) for k, v in R.build(R.RELEASED, "meta").state_dict().items()}
    assert got == want["state_dict"], (sorted(set(got) ^ set(want["state_dict"]))[:8], [k for k in got if k in want["state_dict"] and got[k] != want["state_dict"][k]][:8])
    assert len(got) == 526 and sum(int(np.prod(s)) for s in got.values()) == 600432520


@pytest.fixture(scope="module")
def gold():
    return np.load(R.GOLD)


def test_golden_file_holds_data_only(gold):
    assert json.loads(bytes(gold["cfg_json"]).decode()) == R.SMALL
    assert not [k for k in gold.files if k.startswith("sd") or "weight" in k]
    coords, feats, t, cond = R.golden_inputs()
    assert np.array_equal(gold["coords"], coords.numpy()) and np.array_equal(gold["feats"], feats.numpy())
    assert np.array_equal(gold["t"], t.numpy()) and np.array_equal(gold["cond"], cond.numpy())
    w = R.make_weights(R.SMALL, 3)
    zero_init = [k for k in w if ".conv2." in k or "adaLN_modulation" in k or k.startswith("out_layer")]
    assert len(zero_init) == 4 * 2 + 2 * 2 + 2 and all(float(np.abs(w[k]).max()) > 0 for k in w)


def test_torch_route_reproduces_the_reference(gold):
    model = R.load_weights(R.build(R.SMALL), R.make_weights(R.SMALL, 3))
    coords, feats, t, cond = R.golden_inputs()
    taps = {}
    out = R.run(model, coords, feats, t, cond, R.TorchOps(torch.float32), taps)
    names = [k[4:] for k in gold.files if k.startswith("tap.")]
    assert set(names) == {"input", "in0", "in0_conv1", "in1", "in1_conv1", "block0", "block1", "out0", "out1"}
    for k in names:
        assert taps[k].shape == gold["tap." + k].shape, k
        err = float(np.abs(taps[k].numpy() - gold["tap." + k]).max())
        assert err < 2e-5, (k, err)
    assert float(np.abs(out.numpy() - gold["out"]).max()) < 2e-5


def test_torch_route_keeps_samples_apart(gold):
    """A sample's rows do not depend on what else is in the batch (per-sample modulation, attention and neighbourhoods)."""
    model = R.load_weights(R.build(R.SMALL), R.make_weights(R.SMALL, 3))
    n0 = int((gold["coords"][:, 0] == 0).sum())
    for k, rows in ((0, slice(0, n0)), (1, slice(n0, None))):
        c, f, t, cond = R.golden_inputs(samples=(k,))
        out = R.run(model, c, f, t, cond, R.TorchOps(torch.float32))
        assert float(np.abs(out.numpy() - gold["out"][rows]).max()) < 2e-5


@pytest.mark.parametrize("name", list(R.SAMPLER_CASES))
def test_samplers_reproduce_the_reference_trajectories(gold, name):
    case = R.SAMPLER_CASES[name]
    noise, cond, neg = R.sampler_inputs()
    calls = []

    def model(x, t, c):
        calls.append((float(t[0]), c is neg))
        return R.standin_model(x, t, c)
    s = getattr(smp, case["cls"])(sigma_min=1e-5)
    kw = dict(case["kw"], verbose=False)
    if case.get("neg"):
        kw["neg_cond"] = neg
    ret = s.sample(model, noise, cond, **kw)
    assert set(ret) == {"samples", "pred_x_t", "pred_x_0"} and len(ret.pred_x_t) == len(ret.pred_x_0) == kw["steps"]
    for field, got in (("samples", ret.samples), ("pred_x_t", torch.stack(ret.pred_x_t)), ("pred_x_0", torch.stack(ret.pred_x_0))):
        assert float(np.abs(got.numpy() - gold[f"sampler.{name}.{field}"]).max()) <= 1e-6, field
    assert ret.samples is ret.pred_x_t[-1]
    ts = smp.FlowEulerSampler.timesteps(kw["steps"], kw["rescale_t"])[:-1]
    if name == "interval":          # guidance inside [0.5, 0.95] only: t = 1 and the late steps call the model once
        inside = [0.5 <= t <= 0.95 for t in ts]
        assert any(inside) and not all(inside) and not inside[0]
        assert len(calls) == len(ts) + sum(inside) and sum(n for _, n in calls) == sum(inside)
    elif name == "cfg":
        assert len(calls) == 2 * len(ts)
    else:
        assert len(calls) == len(ts)
    assert [round(c[0], 2) for c in calls if not c[1]] == [round(1000 * float(t), 2) for t in ts]       # the model sees 1000 t


def test_one_map_per_resolution_and_one_context_projection_per_condition():
    """Over a guided 4-step run through the torch operator set: the neighbour-map builder runs twice (16^3 rows, 8^3 rows) although the rows
    that come back from SparseUpsample carry the downsampled rows' scale, and every block projects each condition tensor once."""
    built = []

    class Counting(R.TorchOps):
        def neighbor_map(self, coords):
            built.append(coords.shape[0])
            return R.TorchOps.neighbor_map(coords)
    model = R.load_weights(R.build(R.SMALL), R.make_weights(R.SMALL, 3))
    coords, feats, _, cond = R.golden_inputs()
    neg = torch.zeros_like(cond)
    params = dict(steps=4, cfg_strength=3.0, cfg_interval=(0.5, 1.0), rescale_t=3.0)
    ops = Counting(torch.float32)
    out = smp.sample_slat(model, cond, neg, coords, params, None, noise=feats, ops=ops)
    assert sorted(built) == sorted([coords.shape[0], 88]) and torch.isfinite(out.feats).all()
    assert [b.kv_projections for b in model.blocks] == [2, 2]           # over 8 model calls: t = 1, 0.9, 0.75, 0.5 are all guided


def test_sample_slat_denormalises_and_keeps_the_cache():
    """sample_slat on a stand-in flow model: the SparseTensor state keeps coordinates, layout and spatial cache from step to step, and the
    result is samples * std + mean."""
    coords, feats, _, _ = R.golden_inputs()
    seen = []

    class Flow:
        in_channels = 8

        def __call__(self, x, t, cond):
            seen.append(x)
            x.register_spatial_cache("probe", len(seen)) if x.get_spatial_cache("probe") is None else None
            return x.replace(0.5 * x.feats + cond[x.coords[:, 0].long(), 0, :8])
    cond, neg = torch.ones((2, 3, 8)), torch.zeros((2, 3, 8))
    norm = dict(mean=[0.1 * i for i in range(8)], std=[1.0 + i for i in range(8)])
    params = dict(steps=4, cfg_strength=3.0, cfg_interval=(0.5, 1.0), rescale_t=3.0)
    out = smp.sample_slat(Flow(), cond, neg, coords, params, norm, noise=feats)
    raw = smp.sample_slat(Flow(), cond, neg, coords, params, None, noise=feats)
    assert isinstance(out, sp.SparseTensor) and out.feats.shape == feats.shape and torch.equal(out.coords, coords)
    want = raw.feats * torch.tensor(norm["std"])[None] + torch.tensor(norm["mean"])[None]
    assert float((out.feats - want).abs().max()) < 1e-6
    assert all(s.get_spatial_cache("probe") == 1 for s in seen[:6]) and seen[0]._spatial_cache is seen[5]._spatial_cache
