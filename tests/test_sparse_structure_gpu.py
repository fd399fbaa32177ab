"""The sparse-structure stage on the device (gvfdiffusion_amd/trellis/models/sparse_structure_flow.py and sparse_structure_vae.py on
csrc/conv3d.hip and the existing GEMM / attention / LayerNorm kernels): the small golden configs against the float64 run of the same route,
per stage, within twice the deviation of the torch operator set run on the CPU at the same operand placement (the margin every 16-bit route
of this project gets); the coords of a guided sampling run against the float64 route's; one context projection per condition tensor;
tokens_to_gaussians through sample_slat and SLatGaussianDecoder; the released-size models once."""
import json
import os

import numpy as np
import pytest
import torch

import conv3d_ref as C
import slat_flow_ref as SF
import sparse_structure_ref as R
from gvfdiffusion_amd.trellis import models as tm
from gvfdiffusion_amd.trellis.pipelines import sample_sparse_structure, tokens_to_gaussians

pytestmark = pytest.mark.gpu
DTYPES = [torch.bfloat16, torch.float16]


@pytest.fixture(scope="module")
def small():
    return dict(dec=R.load_weights(R.build_decoder(R.DEC_SMALL), 4), p1=R.load_weights(R.build_flow(R.FLOW_SMALL["p1"]), 3),
                p2=R.load_weights(R.build_flow(R.FLOW_SMALL["p2"]), 3))


@pytest.fixture(scope="module")
def cpu_runs(small):
    """name -> float64 stages; (name, dtype) -> the torch operator set's stages at 16-bit operands.  Computed once, never modified."""
    out = {}
    for dt in [torch.float64] + DTYPES:
        key = (lambda n: n) if dt is torch.float64 else (lambda n: (n, dt))
        wide = (lambda t: t.double()) if dt is torch.float64 else (lambda t: t)
        taps = {}
        R.run_decoder(small["dec"], wide(R.decoder_input()), R.TorchOps(dt), taps)
        out[key("dec")] = taps
        for name in R.FLOW_SMALL:
            x, t, cond = R.flow_inputs(name)
            taps = {}
            taps["y"] = small[name](wide(x), t, wide(cond), ops=R.TorchOps(dt), taps=taps)
            out[key(name)] = taps
        out[key("pipe")] = R.pipeline_logits(small["p1"], small["dec"], R.TorchOps(dt), torch.float64 if dt is torch.float64 else torch.float32)[1]
    return out


def _on_device(models, cuda, dt):
    for m in models:
        m.to(cuda).set_compute_dtype(dt)


def _back(models):
    for m in models:
        m.to("cpu").set_compute_dtype(None)


def _stages(what, dt, taps, ref, host, stages):
    worst = 0.0
    for k in stages:
        dev = float((taps[k].cpu().double() - ref[k]).abs().max())
        yard = float((host[k].double() - ref[k]).abs().max())
        worst = max(worst, dev / yard)
        print(f"{what} {dt} {k}: device {dev:.3e}, torch operators {yard:.3e}, ratio {dev / yard:.2f}")
        assert torch.isfinite(taps[k]).all() and dev <= 2.0 * yard, (k, dev, yard)
    print(f"{what} {dt}: worst ratio {worst:.2f}")


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
def test_small_decoder_stage_by_stage(cuda, small, cpu_runs, dt):
    dec = small["dec"]
    _on_device([dec], cuda, dt)
    try:
        taps = {}
        logits = R.run_decoder(dec, R.decoder_input().to(cuda), None, taps)
        dense = dec(R.decoder_input().to(cuda))
        torch.cuda.synchronize()
    finally:
        _back([dec])
    ref, host = cpu_runs["dec"], cpu_runs["dec", dt]
    assert list(taps) == R.DEC_STAGES == list(ref)
    _stages("sparse-structure decoder", dt, taps, ref, host, R.DEC_STAGES)
    assert logits.dtype == torch.float32 and logits.shape == (1024, 1) and dense.shape == (2, 1, 8, 8, 8)
    assert torch.equal(C.to_rows(dense), logits), "forward() and forward_rows() are one route: equal bits"
    gold = torch.from_numpy(np.load(R.GOLD)["dec.logits"]).double()            # the reference's own fp32 output, at the tolerance of a 16-bit route
    yard = float((host["logits"].double() - ref["logits"]).abs().max())
    assert float((dense.cpu().double() - gold).abs().max()) <= 2.0 * yard + 2e-5


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("name", ["p1", "p2"])
def test_small_flow_model_stage_by_stage(cuda, small, cpu_runs, dt, name):
    model = small[name]
    _on_device([model], cuda, dt)
    try:
        x, t, cond = R.flow_inputs(name)
        taps = {}
        taps["y"] = model(x.to(cuda), t.to(cuda), cond.to(cuda), taps=taps)
        torch.cuda.synchronize()
    finally:
        _back([model])
    ref, host = cpu_runs[name], cpu_runs[name, dt]
    assert list(taps) == R.FLOW_STAGES + ["y"] == list(ref)
    _stages(f"sparse-structure flow {name}", dt, taps, ref, host, R.FLOW_STAGES + ["y"])
    assert taps["y"].shape == x.shape and taps["y"].dtype == torch.float32
    gold = torch.from_numpy(np.load(R.GOLD)[f"flow.{name}.y"]).double()
    assert float((taps["y"].cpu().double() - gold).abs().max()) <= 2.0 * float((host["y"].double() - ref["y"]).abs().max()) + 2e-5


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
def test_coords_of_a_guided_run(cuda, small, cpu_runs, dt):
    """Device coords equal the float64 route's except at cells whose float64 logit is within 2 x the yardstick of zero; those may go either
    way and number at most 1 % of the grid (the float64 side of that cap: tests/test_sparse_structure_host.py).  One context projection per
    block and condition tensor, whatever the step count."""
    flow, dec = small["p1"], small["dec"]
    _on_device([flow, dec], cuda, dt)
    try:
        x, _, cond = R.flow_inputs("p1")
        cond = cond.to(cuda)
        neg = torch.zeros_like(cond)
        kv0 = [b.kv_projections for b in flow.blocks]
        coords = sample_sparse_structure(flow, dec, cond, neg, 2, R.PIPE_PARAMS, noise=x.to(cuda))
        torch.cuda.synchronize()
        assert [b.kv_projections - k for b, k in zip(flow.blocks, kv0)] == [2, 2], "to_kv runs once per block and condition tensor"
        drawn = sample_sparse_structure(flow, dec, cond, neg, 2, dict(R.PIPE_PARAMS, steps=2))             # noise drawn inside
        assert [b.kv_projections - k for b, k in zip(flow.blocks, kv0)] == [2, 2], "a second run reuses the projected context"
    finally:
        _back([flow, dec])
    for c in (coords, drawn):
        assert c.is_cuda and c.dtype == torch.int32 and c.dim() == 2 and c.shape[1] == 4
    c = coords.cpu().long()
    assert bool((c >= 0).all()) and bool((c[:, 0] < 2).all()) and bool((c[:, 1:] < 8).all())
    rows = ((c[:, 0] * 8 + c[:, 1]) * 8 + c[:, 2]) * 8 + c[:, 3]
    assert bool((rows[1:] > rows[:-1]).all()), "coords are unique and in row order"
    ref, host = cpu_runs["pipe"].reshape(-1), cpu_runs["pipe", dt].reshape(-1)
    yard = float((host.double() - ref).abs().max())
    free = ref.abs() <= 2.0 * yard
    assert int(free.sum()) <= ref.numel() // 100
    got = torch.zeros(ref.numel(), dtype=torch.bool)
    got[rows] = True
    differ = (got != (ref > 0)) & ~free
    print(f"sparse structure {dt}: {coords.shape[0]} cells occupied, yardstick {yard:.3e}, {int(free.sum())} cells free to go either way, "
          f"{int((got != (ref > 0)).sum())} differ from float64")
    assert int(differ.sum()) == 0 and 5 <= coords.shape[0] <= 60


@pytest.mark.parametrize("store", ["rows", "shuffle2"])
def test_wide_full_grids_route_through_the_submanifold_kernel(cuda, store):
    """HipOps.dense_conv3 sends a convolution whose channel counts are multiples of 64 to gvf_spconv3 on the full grid's neighbour map once
    that launch fills the card; the result is the same operator: every element within conv3d_ref's bound (the k-step
    count is the same, 27 ceil(Cin / 32)), bias, addend and the pixel-shuffle included.  (4, 16, 16, 16), 64 -> 64: 256 workgroups."""
    from gvfdiffusion_amd.trellis.models.structured_latent_flow import HipOps
    grid, cin, cout, dt = (4, 16, 16, 16), 64, 64, torch.float16
    assert HipOps.spconv_route(4 * 16 ** 3, cin, cout) and not HipOps.spconv_route(4 * 16 ** 3 - 64, cin, cout)
    assert not HipOps.spconv_route(1 << 20, 32, 64) and not HipOps.spconv_route(1 << 20, 64, 8) and HipOps.spconv_route(32 ** 3, 128, 256)
    x16, w16, w32, bias, addend = C.make_operands(grid, cin, cout, dt, seed=51, store=store)
    conv = torch.nn.Conv3d(cin, cout, 3, padding=1)
    conv.load_state_dict({"weight": w32, "bias": bias})
    conv = conv.to(cuda)
    ops = HipOps(dt)
    out = ops.dense_conv3(x16.to(cuda), grid, conv, addend=addend.to(cuda), store=store)
    again = ops.dense_conv3(x16.to(cuda), grid, conv, addend=addend.to(cuda), store=store)
    torch.cuda.synchronize()
    assert any(k[0] == "full_grid_map" for k in ops.cache if isinstance(k, tuple)) and torch.equal(out, again)
    ref, bnd = C.model(x16, grid, w16, bias, addend, None, store)
    n_bad, worst = C.excess(out.cpu(), ref, bnd)
    print(f"routed dense conv {store}: worst |err| / bound {worst:.3f}")
    assert out.dtype == torch.float32 and out.shape == ref.shape and n_bad == 0


def test_tokens_to_gaussians_end_to_end(cuda, small):
    z = np.load(os.path.join(os.path.dirname(__file__), "golden", "slat_decoder_golden.npz"))
    cfg = json.loads(bytes(z["cfg_json"]).decode())
    torch.manual_seed(3)
    gs = tm.SLatGaussianDecoder(**cfg)
    torch.nn.init.normal_(gs.out_layer.weight, std=0.02)
    slat_flow = SF.load_weights(SF.build(SF.SMALL), SF.make_weights(SF.SMALL, 3))
    models = {"sparse_structure_flow_model": small["p1"], "sparse_structure_decoder": small["dec"], "slat_flow_model": slat_flow}
    _on_device(models.values(), cuda, torch.float16)
    models["slat_decoder_gs"] = gs.to(cuda)
    try:
        x, _, cond = R.flow_inputs("p1")
        cond = cond.to(cuda)
        torch.manual_seed(11)
        reps, slat, coords = tokens_to_gaussians(models, cond, torch.zeros_like(cond), 2, R.PIPE_PARAMS, R.PIPE_PARAMS,
                                                 dict(mean=[0.05 * i for i in range(8)], std=[1.0 + 0.1 * i for i in range(8)]), noise=x.to(cuda))
        torch.cuda.synchronize()
    finally:
        _back([small["p1"], small["dec"]])
    assert coords.dtype == torch.int32 and coords.shape[0] >= 1 and slat.feats.shape == (coords.shape[0], 8)
    lens = [int((coords[:, 0] == b).sum()) for b in range(2)]
    n = cfg["representation_config"]["num_gaussians"]
    assert len(reps) == 2 and min(lens) >= 1 and sum(lens) == coords.shape[0]          # the golden noise: both samples have occupied cells
    for g, L in zip(reps, lens):
        assert g.get_xyz.shape == (L * n, 3)
        for v in (g.get_xyz, g.get_scaling, g.get_opacity, g._rotation):
            assert torch.isfinite(v).all()


def test_released_size_flow_model_runs_once(cuda):
    torch.manual_seed(1)
    with torch.device(cuda):
        model = tm.SparseStructureFlowModel(**R.FLOW_RELEASED).eval()
        for b in model.blocks:
            torch.nn.init.normal_(b.adaLN_modulation[1].weight, std=0.01)
        torch.nn.init.normal_(model.out_layer.weight, std=0.05)
    g = torch.Generator().manual_seed(2)
    x = torch.randn((1, 8, 16, 16, 16), generator=g).to(cuda)
    cond = torch.randn((1, 1374, 1024), generator=g).to(cuda)
    y = model(x, torch.tensor([500.0], device=cuda), cond)
    torch.cuda.synchronize()
    assert y.shape == x.shape and y.dtype == torch.float32
    assert torch.isfinite(y).all() and float(y.abs().max()) > 0 and float(y.std()) > 0
    assert model._lp() == torch.float16


def test_released_size_decoder_runs_once_into_the_coords(cuda):
    torch.manual_seed(1)
    with torch.device(cuda):
        dec = tm.SparseStructureDecoder(**R.DEC_RELEASED).eval()
        for m in dec.modules():
            if isinstance(m, tm.ResBlock3d):
                torch.nn.init.normal_(m.conv2.weight, std=0.01)
    z = torch.randn((1, 8, 16, 16, 16), generator=torch.Generator().manual_seed(2)).to(cuda)
    logits, grid = dec.forward_rows(C.to_rows(z), (1, 16, 16, 16))
    assert grid == (1, 64, 64, 64) and logits.shape == (64 ** 3, 1) and logits.dtype == torch.float32
    assert torch.isfinite(logits).all() and float(logits.std()) > 0
    from gvfdiffusion_amd.ops import conv3d
    coords = conv3d.occupancy_coords(logits.reshape(1, -1), grid)
    torch.cuda.synchronize()
    assert coords.dtype == torch.int32 and coords.shape == (int((logits > 0).sum()), 4)
    assert 0 < coords.shape[0] < 64 ** 3
    assert torch.equal(coords.long(), torch.argwhere(logits.reshape(1, 64, 64, 64) > 0))
    assert dec._lp() == torch.float16
