"""The structured-latent flow model on the device (gvfdiffusion_amd/trellis/models/structured_latent_flow.py on csrc/spconv.hip and the
existing GEMM / attention / LayerNorm kernels): the small golden config against the float64 run of the same route, per stage, within twice
the deviation of the torch operator set run on the CPU at the same operand placement (the margin every 16-bit route of this project gets);
the module API; one neighbour map per resolution and one context projection per condition over a guided sampling run; sample_slat ->
SLatGaussianDecoder; the released-size model once."""
import json
import os

import numpy as np
import pytest
import torch

import slat_flow_ref as R
import spconv_ref as S
from gvfdiffusion_amd import sparse as sp
from gvfdiffusion_amd.ops import spconv
from gvfdiffusion_amd.trellis import models as tm
from gvfdiffusion_amd.trellis.pipelines import sample_slat

pytestmark = pytest.mark.gpu
DTYPES = [torch.bfloat16, torch.float16]
STAGES = ["input", "in0_conv1", "in0", "in1_conv1", "in1", "block0_self", "block0_cross", "block0", "block1_self", "block1_cross", "block1",
          "out0", "out1", "out"]


@pytest.fixture(scope="module")
def small():
    return R.load_weights(R.build(R.SMALL), R.make_weights(R.SMALL, 3))


@pytest.fixture(scope="module")
def cpu_runs(small):
    """(samples) -> float64 stages; (samples, dtype) -> the torch operator set's stages at 16-bit operands.  Computed once, never modified."""
    out = {}
    for samples in ((0, 1), (1,)):
        c, f, t, cond = R.golden_inputs(samples=samples)
        taps = {}
        taps["out"] = R.run(small, c, f.double(), t, cond, R.TorchOps(torch.float64), taps)
        out[samples] = taps
        for dt in DTYPES:
            taps = {}
            taps["out"] = R.run(small, c, f, t, cond, R.TorchOps(dt), taps)
            out[samples, dt] = taps
    return out


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("samples", [(0, 1), (1,)], ids=["two", "one"])
def test_small_config_stage_by_stage(cuda, small, cpu_runs, dt, samples):
    model = small.to(cuda).set_compute_dtype(dt)
    try:
        c, f, t, cond = R.golden_inputs(samples=samples)
        taps = {}
        x = sp.SparseTensor(f.to(cuda), c.to(cuda))
        taps["out"] = model(x, t.to(cuda), cond.to(cuda), taps=taps).feats
        torch.cuda.synchronize()
    finally:
        small.to("cpu").set_compute_dtype(None)
    ref, host = cpu_runs[samples], cpu_runs[samples, dt]
    assert set(taps) == set(STAGES) == set(ref)
    worst = 0.0
    for k in STAGES:
        dev = float((taps[k].cpu().double() - ref[k]).abs().max())
        yard = float((host[k].double() - ref[k]).abs().max())
        worst = max(worst, dev / yard)
        print(f"slat flow {dt} {len(samples)} sample(s) {k}: device {dev:.3e}, torch operators {yard:.3e}, ratio {dev / yard:.2f}")
        assert torch.isfinite(taps[k]).all() and dev <= 2.0 * yard, (k, dev, yard)
    print(f"slat flow {dt} {len(samples)} sample(s): worst ratio {worst:.2f}")
    if samples == (0, 1):           # the reference's own fp32 output, at the tolerance of a 16-bit route
        gold = torch.from_numpy(np.load(R.GOLD)["out"]).double()
        assert float((taps["out"].cpu().double() - gold).abs().max()) <= 2.0 * float((host["out"].double() - ref["out"]).abs().max()) + 2e-5


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
def test_sparse_conv3d_module(cuda, dt):
    """SparseConv3d on a SparseTensor: the operator's bound through the module API, the map cached on the tensor and carried by replace()."""
    coords = S.standard_coords(permuted=True)
    x16, w16, w32, bias, _ = S.make_operands(coords.shape[0], 64, 128, dt, seed=41)
    conv = sp.SparseConv3d(64, 128, 3)
    conv.load_state_dict({"conv.weight": w32, "conv.bias": bias}, strict=True)
    conv = conv.to(cuda)
    x = sp.SparseTensor(x16.to(cuda), coords.to(cuda))
    n0 = spconv.MAP_BUILDS
    y = conv(x)
    y2 = conv(x.replace(x.feats * 2))
    assert spconv.MAP_BUILDS == n0 + 1 and y.dtype == dt and torch.equal(y.coords, x.coords)
    ref, bnd = S.model(x16, S.neighbor_map(coords), w16, bias)            # the module rounds the fp32 result to the tensor's type
    e = S._round_bound(ref, bnd, dt)
    assert S.excess(y.feats.cpu(), ref, e)[0] == 0
    assert torch.isfinite(y2.feats.float()).all()
    k1 = sp.SparseConv3d(64, 32, 1).to(cuda)
    z = k1(x)
    want = x16[:, :64].double() @ k1.conv.weight.detach().cpu().to(dt).double().reshape(32, 64).T + k1.conv.bias.detach().cpu().double()
    assert float((z.feats.cpu().double() - want).abs().max()) <= 2.0 ** (-7 if dt is torch.bfloat16 else -10) * float(want.abs().max())


def test_blocks_through_the_module_api(cuda, small, cpu_runs):
    """SparseResBlock3d and ModulatedSparseTransformerCrossBlock called as modules (t_emb in, SparseTensor out) agree with the model's stages."""
    c, f, t, cond = R.golden_inputs()
    ref = cpu_runs[(0, 1)]
    t_emb = R.TorchOps(torch.float64).t_emb(t, small.t_embedder)
    model = small.to(cuda).set_compute_dtype(torch.float16)
    try:
        x = sp.SparseTensor(ref["input"].float().to(cuda), c.to(cuda))
        y = model.input_blocks[0](x, t_emb.float().to(cuda))
        assert isinstance(y, sp.SparseTensor) and y.feats.dtype == torch.float32
        assert float((y.feats.cpu().double() - ref["in0"]).abs().max()) < 0.02 * float(ref["in0"].abs().max())
        down = model.input_blocks[1](y, t_emb.float().to(cuda))
        assert down.feats.shape == ref["in1"].shape and down.coords.shape[0] < c.shape[0]
        assert float((down.feats.cpu().double() - ref["in1"]).abs().max()) < 0.02 * float(ref["in1"].abs().max())
        pos = model._position_rows(down)
        z = model.blocks[0](down.replace(down.feats + pos), t_emb.float().to(cuda), cond.to(cuda))
        assert float((z.feats.cpu().double() - ref["block0"]).abs().max()) < 0.02 * float(ref["block0"].abs().max())
    finally:
        small.to("cpu").set_compute_dtype(None)


def test_one_map_per_resolution_over_a_sampling_run(cuda, small):
    model = small.to(cuda).set_compute_dtype(torch.float16)
    try:
        c, f, _, cond = R.golden_inputs()
        cond, neg = cond.to(cuda), torch.zeros_like(cond).to(cuda)
        n0, kv0 = spconv.MAP_BUILDS, [b.kv_projections for b in model.blocks]
        params = dict(steps=4, cfg_strength=3.0, cfg_interval=(0.5, 1.0), rescale_t=3.0)
        norm = dict(mean=[0.0] * 8, std=[1.0] * 8)
        slat = sample_slat(model, cond, neg, c.to(cuda), params, norm, noise=f.to(cuda))
        torch.cuda.synchronize()
        assert spconv.MAP_BUILDS - n0 == 2, "one neighbour map for the 16^3 rows and one for the 8^3 rows, whatever the number of steps"
        assert [b.kv_projections - k for b, k in zip(model.blocks, kv0)] == [2, 2], "to_kv runs once per block and condition tensor"
        assert slat.feats.shape == f.shape and torch.isfinite(slat.feats).all()
        # a second run is NOT bit-identical: SparseDownsample pools with index_add_ (float atomics), and a flipped last bit of a pooled row
        # flips 16-bit roundings downstream; it agrees to the size of those
        again = sample_slat(model, cond, neg, c.to(cuda), params, norm, noise=f.to(cuda))
        assert spconv.MAP_BUILDS - n0 == 4, "a new SparseTensor has a new cache: two more maps"
        assert float((again.feats - slat.feats).abs().max()) < 0.05 * float(slat.feats.abs().max())
    finally:
        small.to("cpu").set_compute_dtype(None)


def test_sample_slat_feeds_the_gaussian_decoder(cuda, small):
    z = np.load(os.path.join(os.path.dirname(__file__), "golden", "slat_decoder_golden.npz"))
    cfg = json.loads(bytes(z["cfg_json"]).decode())
    torch.manual_seed(3)
    dec = tm.SLatGaussianDecoder(**cfg)
    torch.nn.init.normal_(dec.out_layer.weight, std=0.02)
    dec = dec.to(cuda)
    model = small.to(cuda).set_compute_dtype(torch.bfloat16)
    try:
        c, f, _, cond = R.golden_inputs()
        slat = sample_slat(model, cond.to(cuda), torch.zeros_like(cond).to(cuda), c.to(cuda), dict(steps=3, cfg_strength=3.0, cfg_interval=(0.5, 1.0), rescale_t=3.0),
                           dict(mean=[0.05 * i for i in range(8)], std=[1.0 + 0.1 * i for i in range(8)]), noise=f.to(cuda))
        reps = dec(slat)
    finally:
        small.to("cpu").set_compute_dtype(None)
    lens = [int((c[:, 0] == b).sum()) for b in range(2)]
    n = cfg["representation_config"]["num_gaussians"]
    assert len(reps) == 2
    for g, L in zip(reps, lens):
        assert g.get_xyz.shape == (L * n, 3)
        for v in (g.get_xyz, g.get_scaling, g.get_opacity, g._rotation):
            assert torch.isfinite(v).all()
    assert float(reps[0].get_xyz.std()) > 0


def test_released_size_model_runs_once(cuda):
    torch.manual_seed(1)
    with torch.device(cuda):
        model = tm.SLatFlowModel(**R.RELEASED).eval()
        for b in model.blocks:
            torch.nn.init.normal_(b.adaLN_modulation[1].weight, std=0.01)
        for b in list(model.input_blocks) + list(model.out_blocks):
            torch.nn.init.normal_(b.conv2.conv.weight, std=0.01)
        torch.nn.init.normal_(model.out_layer.weight, std=0.05)
    coords = S.shell(64, 12.5, 13.5).to(cuda)
    assert 1800 <= coords.shape[0] <= 2400
    g = torch.Generator().manual_seed(2)
    x = sp.SparseTensor(torch.randn((coords.shape[0], 8), generator=g).to(cuda), coords)
    cond = torch.randn((1, 1374, 1024), generator=g).to(cuda)
    y = model(x, torch.tensor([500.0], device=cuda), cond)
    torch.cuda.synchronize()
    assert y.feats.shape == (coords.shape[0], 8) and y.feats.dtype == torch.float32
    assert torch.isfinite(y.feats).all() and float(y.feats.abs().max()) > 0
    assert model._lp() == torch.float16
