"""Host side of the LPIPS operator (include/gvf_lpips.h, gvfdiffusion_amd/ops/lpips.py): size queries, argument errors answered before
any launch, CPU tensors refused, the reference's state-dict names.  No GPU."""
import ctypes
import sys
import types

import pytest
import torch

import lpips_ref as R
from gvfdiffusion_amd import _lib
from gvfdiffusion_amd.ops import lpips as LP


def test_packed_bytes_queries():
    assert LP.packed_bytes(64, 64) == 64 * 64 * 9 * 2
    assert LP.packed_bytes(512, 256, LP.PACK_DGRAD) == 512 * 256 * 9 * 2
    assert LP.packed_bytes(64, 3) == 64 * 32 * 2                      # K = 27 padded to one 32-wide k-step
    l, out = _lib.lib(), ctypes.c_size_t(0)
    for cout, cin, mode in ((64, 3, LP.PACK_DGRAD), (128, 3, LP.PACK_FWD), (96, 64, 0), (64, 32, 0), (1024, 64, 0), (0, 64, 0), (64, -64, 0),
                            (64, 64, 2)):
        assert l.gvf_conv3x3_packed_bytes(cout, cin, mode, ctypes.byref(out)) == _lib.GVF_EINVAL, (cout, cin, mode)
    assert l.gvf_conv3x3_packed_bytes(64, 64, 0, None) == _lib.GVF_EINVAL
    assert l.gvf_lpips_tap_scratch_bytes(2, 37, 50, ctypes.byref(out)) == 0 and out.value >= 2 * 8
    for n, h, w in ((0, 8, 8), (1, 0, 8), (1, 8, -1)):
        assert l.gvf_lpips_tap_scratch_bytes(n, h, w, ctypes.byref(out)) == _lib.GVF_EINVAL


def test_bad_arguments_are_refused_before_any_launch():
    """Pointers are never dereferenced on the host: dummy non-null, 16-byte aligned addresses stand in for device memory."""
    l, p = _lib.lib(), ctypes.c_void_p(0x1000)
    ok = dict(N=1, H=8, W=8, cin=64, cout=64, flags=0, dtype=0)

    def conv(**kw):
        a = {**ok, **kw}
        return l.gvf_conv3x3(p, p, None, None, None, p, a["N"], a["H"], a["W"], a["cin"], a["cout"], a["flags"], a["dtype"], None)

    for bad in (dict(cin=96), dict(cout=32), dict(cin=3), dict(dtype=2), dict(dtype=-1), dict(N=0), dict(H=0), dict(W=-3), dict(flags=2)):
        assert conv(**bad) == _lib.GVF_EINVAL, bad
    assert l.gvf_conv3x3(None, p, None, None, None, p, 1, 8, 8, 64, 64, 0, 0, None) == _lib.GVF_EINVAL
    assert l.gvf_conv3x3(p, p, None, None, None, ctypes.c_void_p(0x1004), 1, 8, 8, 64, 64, 0, 0, None) == _lib.GVF_EINVAL     # misaligned
    assert l.gvf_conv3x3_pack(p, 64, 64, 0, 5, p, 1 << 20, None) == _lib.GVF_EINVAL
    assert l.gvf_conv3x3_pack(p, 64, 64, 0, 0, p, 16, None) == _lib.GVF_ENOSPC
    assert l.gvf_lpips_first_forward(p, p, p, p, p, p, 1, 8, 0, 0, None) == _lib.GVF_EINVAL
    assert l.gvf_lpips_first_forward(p, p, p, p, p, p, 1, 8, 8, 3, None) == _lib.GVF_EINVAL
    assert l.gvf_lpips_first_backward(p, p, p, p, 0, 8, 8, None) == _lib.GVF_EINVAL
    assert l.gvf_maxpool2x2_forward(p, p, 1, 1, 8, 64, 0, None) == _lib.GVF_EINVAL          # nothing to pool
    assert l.gvf_maxpool2x2_forward(p, p, 1, 8, 8, 12, 0, None) == _lib.GVF_EINVAL
    assert l.gvf_maxpool2x2_backward(p, p, p, p, 1, 8, 8, 64, 9, None) == _lib.GVF_EINVAL
    assert l.gvf_lpips_tap_forward(p, p, p, 1, 8, 8, 96, 0, p, p, 1 << 20, None) == _lib.GVF_EINVAL
    assert l.gvf_lpips_tap_forward(p, p, p, 1, 8, 8, 64, 0, p, p, 0, None) == _lib.GVF_ENOSPC
    assert l.gvf_lpips_tap_backward(p, p, p, p, 1, 8, 8, 64, 0, 4, p, None) == _lib.GVF_EINVAL
    assert l.gvf_lpips_tap_backward(p, p, p, p, 1, -8, 8, 64, 0, 0, p, None) == _lib.GVF_EINVAL


def test_cpu_tensors_and_bad_shapes_are_refused():
    m = LP.LPIPS()
    x = torch.zeros((1, 3, 16, 16))
    with pytest.raises(_lib.GvfError):
        m(x, x)
    with pytest.raises(_lib.GvfError):
        LP.pack_conv(torch.zeros((64, 64, 3, 3)), LP.PACK_FWD, torch.float16)
    with pytest.raises(_lib.GvfError):
        LP.conv3x3(torch.zeros((1, 4, 4, 64), dtype=torch.float16), torch.zeros(8, dtype=torch.uint8), 64)
    with pytest.raises(_lib.GvfError):
        LP.tap_forward(torch.zeros((1, 4, 4, 64), dtype=torch.float16), torch.zeros((1, 4, 4, 64), dtype=torch.float16), torch.ones(64))
    with pytest.raises(TypeError):
        m(x, None)
    with pytest.raises(ValueError):
        LP.LPIPS(dtype=torch.float32)
    with pytest.raises(ValueError):
        LP.LPIPS(chunk=0)


def test_the_reference_state_dict_loads():
    m = LP.LPIPS()
    assert all(not p.requires_grad for p in m.parameters())
    sd = R.seeded_weights(3)
    keys = [f"net.layers.{i}.{n}" for i in (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28) for n in ("weight", "bias")] + \
           ["net.mean", "net.std"] + [f"lin.{t}.1.weight" for t in range(5)]
    assert sorted(sd) == sorted(keys) == sorted(m.state_dict())
    before = m.net.layers["28"].weight.clone()
    m.load_state_dict(sd, strict=True)
    assert torch.equal(m.net.layers["28"].weight, sd["net.layers.28.weight"]) and not torch.equal(before, sd["net.layers.28.weight"])
    assert m.lin[4][1].weight.shape == (1, 512, 1, 1) and m.net.mean.shape == (1, 3, 1, 1)
    # two fresh modules start from the same deterministic initialisation
    assert torch.equal(LP.LPIPS().net.layers["0"].weight, LP.LPIPS().net.layers["0"].weight)


def test_render_loss_frames_defaults_do_not_touch_lpips(monkeypatch):
    """With the default arguments render_loss_frames is the L1 + SSIM loss alone: it runs with ops.lpips made unimportable."""
    import gvfdiffusion_amd.ops as ops
    from gvfdiffusion_amd import training
    from gvfdiffusion_amd.ops import image_loss as IL
    monkeypatch.delattr(ops, "lpips")
    monkeypatch.setitem(sys.modules, "gvfdiffusion_amd.ops.lpips", None)        # `import` of it now raises ImportError
    with pytest.raises(ImportError):
        from gvfdiffusion_amd.ops import lpips  # noqa: F401
    seen = {}

    def fake_image_loss(imgs, targets, l1_weight, ssim_weight):
        seen["w"] = (l1_weight, ssim_weight)
        return (imgs - targets).abs().mean()

    monkeypatch.setattr(IL, "image_loss", fake_image_loss)
    frames = torch.full((2, 3, 4, 4), 0.5)
    rend = types.SimpleNamespace(render_frames=lambda *a, **k: {"rgb": frames})
    v = training.render_loss_frames(rend, None, torch.zeros((2, 4, 4)), None, None, torch.zeros((2, 3, 4, 4)))
    assert float(v) == 0.5 and seen["w"] == (1.0, 0.2)
    # and with a module and a weight the term is added on the same frames, scaled to [-1, 1]
    calls = []

    def fake_lpips(a, b):
        calls.append((a, b))
        return torch.tensor(2.0)

    v = training.render_loss_frames(rend, None, torch.zeros((2, 4, 4)), None, None, torch.zeros((2, 3, 4, 4)), lpips=fake_lpips, lpips_weight=0.25)
    assert float(v) == 1.0 and float(calls[0][0].max()) == 0.0 and float(calls[0][1].min()) == -1.0
    assert float(training.render_loss_frames(rend, None, torch.zeros((2, 4, 4)), None, None, torch.zeros((2, 3, 4, 4)), lpips=fake_lpips)) == 0.5
