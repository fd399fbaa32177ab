"""Host side of a projection's backward (include/gvf_linear_grad.h, gvfdiffusion_amd/ops/linear_grad.py, the `linear=` route of
model/dit_train.py): the header, the exports and the ctypes signatures agree, every argument error is answered with GVF_EINVAL before any launch,
the split rule and the workspace size are the documented functions of the extents, the public switch validates its argument, and the
`linear_params` seam of forward_train is wired like the `linear` one (CPU, fp32, through the torch namespace).  No GPU needed: nothing here
reaches a launch."""
import ctypes
import os
import re

import pytest
import torch
import torch.nn.functional as F

import dit_train_ref as R
from gvfdiffusion_amd import _build, _lib
from gvfdiffusion_amd.model import dit_train
from gvfdiffusion_amd.ops import linear_grad

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E = _lib.GVF_EINVAL
NAMES = ("gvf_cast_transpose", "gvf_gemm_wgrad_splits", "gvf_gemm_wgrad_workspace_bytes", "gvf_gemm_wgrad")


def test_header_exports_and_signatures_agree():
    src = open(os.path.join(ROOT, "include", "gvf_linear_grad.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    decl = {m.group(1): m.group(2) for m in re.finditer(r"\bint\s+(gvf_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src)}
    assert set(decl) == set(NAMES)
    raw = ctypes.CDLL(_build.LIB_PATH)
    for name in NAMES:
        assert hasattr(raw, name), f"{name} declared but not exported"
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int
        params = [p.strip() for p in decl[name].split(",")]
        assert len(params) == len(args), f"{name}: {len(params)} parameters declared, {len(args)} in the ctypes signature"
        for p, a in zip(params, args):
            if "size_t*" in p.replace(" *", "*"):
                want = ctypes.POINTER(ctypes.c_size_t)
            elif "*" in p:
                want = ctypes.c_void_p
            elif p.startswith("size_t"):
                want = ctypes.c_size_t
            else:
                want = ctypes.c_int
            assert a is want or a == want, f"{name}: parameter '{p}' bound as {a}"
    assert "linear_grad.hip" in _build.SOURCES and _build.SOURCES["linear_grad.hip"] == _build.SOURCES["gemm.hip"]


def _wgrad(dtype=0, dy=0x10000, ldy=192, x=0x20000, ldx=64, M=240, N=192, K=64, dw=0x30000, lddw=64, db=0x40000, ws=0x100000, ws_bytes=None,
           splits=0):
    l = _lib.lib()
    if ws_bytes is None:
        ws_bytes = 1 << 30
    return l.gvf_gemm_wgrad(dtype, dy, ldy, x, ldx, M, N, K, dw, lddw, db, ws, ws_bytes, splits, None)


@pytest.mark.parametrize("over", [
    dict(dtype=2), dict(dtype=-1),                                         # not a 16-bit type
    dict(dy=None), dict(x=None), dict(dw=None), dict(ws=None),             # null pointers (db alone is optional)
    dict(ldy=184), dict(ldx=56), dict(lddw=56),                            # leading dimension below the extent
    dict(ldy=196), dict(ldx=68), dict(lddw=68),                            # ... not a multiple of 8
    dict(splits=-1), dict(splits=1 << 20),
    dict(ws_bytes=0), dict(ws_bytes=(192 * 64 + 192) * 4 - 1, splits=1), dict(ws_bytes=2 * (192 * 64 + 192) * 4 - 1, splits=2),
    dict(M=-1), dict(N=0), dict(K=0), dict(N=196, ldy=200), dict(K=60),    # extents: M >= 0, N and K positive multiples of 8
    dict(dy=0x10008), dict(x=0x20002), dict(dw=0x30004), dict(db=0x40004), dict(ws=0x100008),      # 16-byte alignment
], ids=lambda o: ",".join(f"{k}={v}" for k, v in o.items()))
def test_wgrad_refuses_bad_arguments_on_the_host(over):
    assert _wgrad(**over) == E


def test_cast_transpose_refuses_bad_arguments_on_the_host():
    l = _lib.lib()
    ct = lambda dtype=0, w=0x10000, ldw=64, w16=0x20000, ld_k=64, w16t=0x30000, ld_n=192, N=192, K=64: \
        l.gvf_cast_transpose(dtype, w, ldw, w16, ld_k, w16t, ld_n, N, K, None)
    for over in (dict(dtype=3), dict(w=None), dict(w16=None), dict(w16t=None), dict(ldw=63), dict(ld_k=56), dict(ld_n=184), dict(ld_k=68),
                 dict(ld_n=196), dict(N=0), dict(K=0), dict(N=-8), dict(w=0x10002), dict(w16=0x20002), dict(w16t=0x30001)):
        assert ct(**over) == E, over


def test_splits_is_a_pure_function_of_the_extents():
    l = _lib.lib()
    CUS, MAX_AUTO, MIN_STEPS = 256, 16, 8

    def rule(M, N, K):
        """include/gvf_linear_grad.h: two workgroups per CU over the output tiles, at most 16 slots, at least 8 k-steps per group"""
        tiles = -(-N // 128) * -(-K // 128)
        steps = -(-M // 32)
        return max(1, min(2 * CUS // tiles, MAX_AUTO, steps // MIN_STEPS))

    shapes = [(0, 64, 64), (1, 32, 32), (240, 192, 64), (257, 2048, 512), (4099, 512, 512), (12288, 512, 512), (12288, 1536, 512),
              (12288, 2048, 512), (12288, 512, 2048), (24 * 1370, 1024, 512), (24 * 4096, 1024, 512), (1000, 160, 288), (1 << 30, 8, 8)]
    for M, N, K in shapes:
        s = l.gvf_gemm_wgrad_splits(M, N, K)
        assert s == rule(M, N, K) and s >= 1, (M, N, K, s)
        assert l.gvf_gemm_wgrad_splits(M, N, K) == s                       # asked again: the same
        assert linear_grad.wgrad_splits(M, N, K) == s
    assert l.gvf_gemm_wgrad_splits(12288, 512, 512) == 16 and l.gvf_gemm_wgrad_splits(4099, 512, 512) == 16
    assert l.gvf_gemm_wgrad_splits(12288, 1536, 512) == 10 and l.gvf_gemm_wgrad_splits(12288, 2048, 512) == 8 and l.gvf_gemm_wgrad_splits(240, 192, 64) == 1
    for bad in ((-1, 64, 64), (8, 0, 64), (8, 64, -8)):
        assert l.gvf_gemm_wgrad_splits(*bad) == E


def test_workspace_bytes():
    l = _lib.lib()
    up = lambda v: (v + 255) // 256 * 256
    for M, N, K, splits in [(1, 32, 32, 1), (33, 192, 64, 2), (1000, 160, 288, 7), (40, 128, 128, 4), (4099, 512, 512, 0), (240, 64, 256, 0)]:
        nb = ctypes.c_size_t(0)
        assert l.gvf_gemm_wgrad_workspace_bytes(M, N, K, splits, ctypes.byref(nb)) == _lib.GVF_OK
        s = splits if splits else l.gvf_gemm_wgrad_splits(M, N, K)
        assert nb.value == up(s * (N * K + N) * 4), (M, N, K, splits)
        assert linear_grad.wgrad_workspace_bytes(M, N, K, splits) == nb.value
    nb = ctypes.c_size_t(0)
    assert l.gvf_gemm_wgrad_workspace_bytes(8, 8, 8, 1, None) == E
    for bad in ((-1, 8, 8, 1), (8, 0, 8, 1), (8, 8, 0, 1), (8, 8, 8, -1), (8, 8, 8, 1 << 20)):
        assert l.gvf_gemm_wgrad_workspace_bytes(*bad, ctypes.byref(nb)) == E


def test_operator_refuses_cpu_tensors_and_odd_extents():
    x = torch.zeros((4, 64), dtype=torch.bfloat16)
    w = torch.zeros((96, 64))
    with pytest.raises(_lib.GvfError):
        linear_grad.linear(x, w)
    with pytest.raises(_lib.GvfError):
        linear_grad.wgrad(torch.zeros((4, 96), dtype=torch.bfloat16), x)
    with pytest.raises(_lib.GvfError):
        linear_grad.cast_transpose(w)


@pytest.fixture(scope="module")
def small():
    return R.load_small("cpu")


def test_enable_training_validates_the_route_and_defaults_to_torch(small):
    model, _, fx = small
    assert model.train_linear == "torch" and model.train_forward is False
    with pytest.raises(ValueError):
        model.enable_training(linear="x")
    assert model.train_forward is False and model.train_linear == "torch"          # a refused call changes nothing
    try:
        assert model.enable_training().train_linear == "torch" and model.train_forward is True
        assert model.enable_training(linear="hip").train_linear == "hip"
    finally:
        model.enable_training(False)
    assert model.train_forward is False and model.train_linear == "torch"
    x, t = torch.from_numpy(fx["x_t"]), torch.from_numpy(fx["t"])
    with pytest.raises(ValueError):
        dit_train.forward_train(model, x, t, ops=R.TorchOps(), dtype=torch.float32, linear="x", **fx["cond"])
    with pytest.raises(_lib.GvfError):                                              # "hip" is the HIP route: a CPU tensor is refused, not rerouted
        dit_train.forward_train(model, x, t, dtype=torch.bfloat16, linear="hip", **fx["cond"])
    assert issubclass(dit_train.HipGemmOps, dit_train.HipOps) and dit_train.HipGemmOps().weight_images == {}
    assert dit_train.HipGemmOps().weight_images is not dit_train.HipGemmOps().weight_images      # one set of images per instance


class _ParamOps(R.TorchOps):
    """TorchOps that takes the master parameters of a projection: what forward_train must hand to an `ops` with linear_params."""

    def __init__(self):
        super().__init__()
        self.calls = 0

    def linear_params(self, x, weight, bias, dtype):
        assert weight.dtype == torch.float32 and weight.requires_grad and dtype == torch.float32
        self.calls += 1
        return F.linear(x, weight, bias)

    @staticmethod
    def linear(x, weight, bias=None):
        raise AssertionError("an ops with linear_params must not be asked for linear")


def _grads(model, diffusion, fx, ops):
    model.zero_grad(set_to_none=True)
    fwd = lambda x, ts, **kw: dit_train.forward_train(model, x, ts, ops=ops, dtype=torch.float32, **kw)
    terms, _ = diffusion.training_losses(fwd, torch.from_numpy(fx["x_start"]), torch.from_numpy(fx["t"]), model_kwargs=fx["cond"],
                                         noise=torch.from_numpy(fx["noise"]))
    loss = terms["loss"].mean()
    loss.backward()
    out = float(loss.detach()), {n: p.grad.clone() for n, p in model.named_parameters()}
    model.zero_grad(set_to_none=True)
    return out


def test_linear_params_seam_is_wired_like_linear(small):
    model, diffusion, fx = small
    loss0, g0 = _grads(model, diffusion, fx, R.TorchOps())
    ops = _ParamOps()
    loss1, g1 = _grads(model, diffusion, fx, ops)
    per_block = 6 + 2 + 2 + (0 if model.blocks[0].no_temporal_attn else 2)       # two cross attentions (to_q, to_kv, to_out), the MLP, spatial (and temporal) to_qkv + to_out
    assert ops.calls == per_block * len(model.blocks)
    assert torch.allclose(torch.tensor(loss1), torch.tensor(loss0), rtol=1e-6, atol=0)
    assert set(g1) == set(g0)
    for n in g0:
        assert torch.allclose(g1[n], g0[n], rtol=1e-5, atol=1e-6 * float(g0[n].abs().max())), n
