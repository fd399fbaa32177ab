"""The DiT forward's call plan on the device (MI355X): what DiT.forward_plan says is what a forward launches, the packed streams exist only
where a plan named them, and a captured graph follows the switches.  tests/test_dit_plan_host.py pins the plan's values themselves."""
import contextlib
import json
import os

import pytest
import torch

from gvfdiffusion_amd import synthetic
from gvfdiffusion_amd.model import dit_plan
from gvfdiffusion_amd.model.dit import DiT
from gvfdiffusion_amd.ops import dit_ops

pytestmark = pytest.mark.gpu
MAN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dit_manifest.json")))
KEYS = ("x", "t", "cond_images", "static_latent", "deformation_position_xyz")


@pytest.fixture(scope="module")
def weights():
    return {k: v for k, v in synthetic.dit_state_dict(MAN["state_dict"], seed=0).items() if not k.startswith("blocks.") or int(k.split(".")[1]) < 2}


def make(cuda, weights, **over):
    net = DiT(**dict(MAN["config"], num_blocks=2, **over))
    net.load_state_dict({k: weights[k] for k in net.state_dict()}, strict=True)       # (a model without temporal attention has fewer tensors)
    return net.to(cuda).eval()


def inputs(cuda, B, T, N):
    i = synthetic.dit_inputs(B=B, T=T, N=N, L_img=70, L_static=130, seed=5)
    return {k: i[k].to(cuda) for k in KEYS}


@contextlib.contextmanager
def counted():
    """Every dit_ops function a plan counts, wrapped: calls per name, and the `prefetch` argument of every attention_tiled call."""
    calls, prefetch = dict.fromkeys(dit_plan.LAUNCH_NAMES, 0), []
    orig = {name: getattr(dit_ops, name) for name in dit_plan.LAUNCH_NAMES}

    def wrap(name):
        def f(*a, **k):
            calls[name] += 1
            if name == "attention_tiled":
                prefetch.append(k.get("prefetch"))
            return orig[name](*a, **k)
        return f
    for name in orig:
        setattr(dit_ops, name, wrap(name))
    try:
        yield calls, prefetch
    finally:
        for name, f in orig.items():
            setattr(dit_ops, name, f)


@pytest.mark.parametrize("B,T,N,over", [
    (2, 3, 48, {}), (1, 3, 64, {}), (1, 5, 64, {}), (1, 5, 40, {}), (1, 5, 48, {}), (1, 2, 96, dict(no_temporal_attn=True)),
    (1, 3, 64, dict(use_rowblock=False)), (1, 3, 64, dict(rowblock_temporal=False)), (1, 3, 64, dict(rowblock_tiled_kv=False)),
    (1, 3, 64, dict(weight_prefetch=False)),
])
def test_the_plan_is_what_runs(cuda, weights, B, T, N, over):
    net = make(cuda, weights, **{k: v for k, v in over.items() if k == "no_temporal_attn"})
    for k, v in over.items():
        if k != "no_temporal_attn":
            setattr(net, k, v)
    inp = inputs(cuda, B, T, N)
    y0 = net(**inp)                          # builds the weight and condition caches (their launches are not the forward's)
    plan = net.forward_plan(B, T, N)
    with counted() as (calls, prefetch):
        y = net(**inp)
    print(f"B={B} T={T} N={N} {over}: {plan.path} {({k: v for k, v in calls.items() if v})}")
    assert calls == dict(plan.launches)
    assert torch.equal(y, y0) and y.shape == (B, T, N, 16) and torch.isfinite(y).all()
    if plan.path == "rowblock":
        # per block: spatial, image, static attention; each touches the packed stream of the row-block launch behind it
        streams = net._wcache["rb"]["blocks"]
        for i, blk in enumerate(streams):
            want = [plan.spatial_prefetch_stream, "s4", "s5"] if plan.prefetch else [None] * 3
            for got, name in zip(prefetch[3 * i:3 * i + 3], want):
                assert got is (None if name is None else blk[name])
        assert set(streams[0]) == set(plan.streams)
    else:
        assert all(p is None for p in prefetch) and "rb" not in net._wcache


def test_streams_are_packed_when_a_plan_first_names_them(cuda, weights):
    net = make(cuda, weights)
    inp = inputs(cuda, 1, 3, 64)
    y1 = net(**inp)
    packed = lambda: [set(b) for b in net._wcache["rb"]["blocks"]]
    assert packed() == [{"s23", "s4", "s5"}] * 2
    kept = net._wcache["rb"]["blocks"][0]["s23"]
    net.rowblock_temporal = False
    y0 = net(**inp)
    assert packed() == [{"s2", "s3", "s23", "s4", "s5"}] * 2 and net._wcache["rb"]["blocks"][0]["s23"] is kept
    assert torch.isfinite(y0).all() and not torch.equal(y0, y1)          # (another summation order: tests/test_rowblock_temporal_gpu.py has the bound)
    net.rowblock_temporal = True
    assert torch.equal(net(**inp), y1)


def test_a_captured_graph_follows_the_switches(cuda, weights):
    """The plan is part of the captured graph's key: a path switch assigned between two graphed forwards is a re-capture.  (Before the plan
    existed the second forward replayed the row-block graph.)"""
    net = make(cuda, weights).enable_graph(True)
    inp = inputs(cuda, 1, 3, 64)
    y1 = net(**inp)
    assert torch.equal(net(**inp), y1)                                   # a replay
    net.use_rowblock = False
    y0 = net(**inp)
    fresh = make(cuda, weights)
    fresh.use_rowblock = False
    assert torch.equal(y0, fresh(**inp))                                 # the unfused launches, eagerly, on an identical model
    assert not torch.equal(y0, y1)
    net.use_rowblock = True
    assert torch.equal(net(**inp), y1)
