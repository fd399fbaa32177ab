"""The attention backward's C ABI on the host (include/gvf_attn_bwd.h): every bad argument is refused with GVF_EINVAL before any launch,
the workspace size has the documented shape, and the operator refuses CPU tensors.  No GPU needed: nothing here reaches a launch."""
import ctypes

import pytest
import torch

from gvfdiffusion_amd import _lib
from gvfdiffusion_amd.ops import attention_grad as AG

_i64 = ctypes.c_int64


def _ws(n_outer, n_inner, Lq, Lk, H, C):
    out = ctypes.c_size_t(0)
    rc = _lib.lib().gvf_attn_bwd_workspace_bytes(n_outer, n_inner, Lq, Lk, H, C, ctypes.byref(out))
    return rc, int(out.value)


def test_workspace_bytes_shape():
    rc, base = _ws(4, 1, 512, 1370, 16, 32)
    assert rc == _lib.GVF_OK and base >= 8 * 4 * 16 * 512
    for N, Lq, H in [(1, 1, 1), (24, 512, 16), (512, 24, 16), (1, 8192, 12), (3, 77, 5)]:
        for C in (32, 64):
            rc, nb = _ws(N, 1, Lq, 130, H, C)
            assert rc == _lib.GVF_OK and nb >= 8 * N * H * Lq
    assert _ws(8, 1, 512, 1370, 16, 32)[1] > base and _ws(4, 1, 1024, 1370, 16, 32)[1] > base and _ws(4, 1, 512, 1370, 32, 32)[1] > base
    assert _ws(2, 2, 512, 1370, 16, 32)[1] == base                   # batch = outer * inner
    assert AG.workspace_bytes(4, 512, 1370, 16, 32) == base


@pytest.mark.parametrize("args", [(0, 1, 8, 8, 2, 32), (2, 0, 8, 8, 2, 32), (2, 1, 0, 8, 2, 32), (2, 1, 8, 0, 2, 32), (2, 1, 8, 8, 0, 32),
                                  (-1, 1, 8, 8, 2, 32), (2, 1, -3, 8, 2, 64), (2, 1, 8, 8, 2, 16), (2, 1, 8, 8, 2, 128), (2, 1, 8, 8, 2, 48)])
def test_workspace_bytes_refuses(args):
    assert _ws(*args)[0] == _lib.GVF_EINVAL
    assert _lib.lib().gvf_attn_bwd_workspace_bytes(2, 1, 8, 8, 2, 32, None) == _lib.GVF_EINVAL


def _call(**over):
    """gvf_attn_bwd with plausible host-side values (the pointers are never dereferenced: every case below is refused first)."""
    N, Lq, Lk, H, C = 2, 40, 72, 2, 32
    a = dict(dtype=1, q=0x10000, k=0x20000, v=0x30000, out=0x40000, dout=0x50000, dq=0x60000, dk=0x70000, dv=0x80000,
             n_outer=N, n_inner=1, Lq=Lq, Lk=Lk, H=H, C=C, scale=C ** -0.5, ws=0x90000, ws_bytes=None,
             qs=(Lq * H * C, 0, H * C, C), ks=(Lk * H * C, 0, H * C, C))
    a.update(over)
    if a["ws_bytes"] is None:
        rc, a["ws_bytes"] = _ws(N, 1, Lq, Lk, H, C)
        assert rc == _lib.GVF_OK
    s4 = lambda s: None if s is None else (_i64 * 4)(*s)
    st = [s4(a.get(n, a["qs"] if n in ("os", "dos", "dqs") else a["ks"])) for n in ("qs", "ks", "vs", "os", "dos", "dqs", "dks", "dvs")]
    vp = lambda x: None if x is None else ctypes.c_void_p(x)
    return _lib.lib().gvf_attn_bwd(a["dtype"], vp(a["q"]), vp(a["k"]), vp(a["v"]), vp(a["out"]), vp(a["dout"]), vp(a["dq"]), vp(a["dk"]),
                                   vp(a["dv"]), a["n_outer"], a["n_inner"], a["Lq"], a["Lk"], a["H"], a["C"], *st, a["scale"], vp(a["ws"]),
                                   a["ws_bytes"], None)


@pytest.mark.parametrize("over", [dict(q=None), dict(k=None), dict(v=None), dict(out=None), dict(dout=None), dict(dq=None), dict(dk=None),
                                  dict(dv=None), dict(ws=None), dict(qs=None), dict(dvs=None),
                                  dict(C=16), dict(C=128), dict(C=0),
                                  dict(dtype=2), dict(dtype=-1), dict(dtype=7),
                                  dict(Lq=0), dict(Lk=0), dict(Lq=-5), dict(n_outer=0), dict(n_inner=0), dict(H=0),
                                  dict(ws_bytes=0), dict(ws_bytes=8 * 2 * 2 * 40 - 1),
                                  dict(scale=0.0), dict(scale=-1.0), dict(scale=float("nan")),
                                  dict(q=0x10002), dict(dk=0x70004), dict(qs=(40 * 64, 0, 60, 32)), dict(dks=(72 * 64, 0, 66, 32))])
def test_backward_refuses_bad_arguments_on_the_host(over):
    assert _call(**over) == _lib.GVF_EINVAL


def test_operator_refuses_cpu_tensors_and_bad_shapes():
    q = torch.zeros((1, 8, 2, 32), dtype=torch.float16, requires_grad=True)
    k = torch.zeros((1, 9, 2, 32), dtype=torch.float16)
    with pytest.raises(_lib.GvfError):
        AG.attention(q, k, k)
    with pytest.raises(_lib.GvfError):
        AG.attention_backward(q.detach(), k, k, q.detach(), q.detach(), 0.2)
    with pytest.raises(ValueError):
        AG.attention(q[0], k, k)
