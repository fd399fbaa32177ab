"""Host side of the fused image loss (include/gvf_loss.h): argument refusals before any launch, scratch sizes, the window taps,
and the Python entry points' refusals of CPU tensors.  No GPU needed."""
import ctypes
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ssim_golden.npz")


@pytest.fixture(scope="module")
def L():
    from gvfdiffusion_amd import _lib
    from gvfdiffusion_amd.ops import image_loss  # noqa: F401  (registers the signatures)
    return _lib.lib()


def _bytes(L, planes, H, W, flags):
    out = ctypes.c_size_t(0)
    rc = L.gvf_image_loss_scratch_bytes(planes, H, W, flags, ctypes.byref(out))
    return rc, out.value


def test_scratch_bytes(L):
    from gvfdiffusion_amd import _lib
    from gvfdiffusion_amd.ops.image_loss import SSIM_GRAD
    n = 72 * 800 * 800
    rc, nograd = _bytes(L, 72, 800, 800, 0)
    assert rc == _lib.GVF_OK
    tiles = 72 * 13 * 50                                   # 64 x 16 tiles
    assert 16 * tiles <= nograd < 16 * tiles + 256         # two double partials per workgroup, no per-pixel storage
    rc, grad = _bytes(L, 72, 800, 800, SSIM_GRAD)
    assert rc == _lib.GVF_OK and grad == nograd + 12 * n   # three fp32 partial maps
    for shape in [(1, 1, 1), (1, 5, 7), (3, 37, 53)]:
        rc, b = _bytes(L, *shape, SSIM_GRAD)
        assert rc == _lib.GVF_OK and b >= 12 * shape[0] * shape[1] * shape[2] + 16


def test_scratch_bytes_refusals(L):
    from gvfdiffusion_amd import _lib
    for args in [(0, 8, 8, 0), (-1, 8, 8, 0), (1, 0, 8, 0), (1, 8, 0, 0), (1, -3, 8, 0), (1, 8, 8, 2), (1, 8, 8, -1),
                 (1 << 50, 1 << 15, 1 << 15, 1), (1 << 40, 8, 8, 0)]:
        assert _bytes(L, *args)[0] == _lib.GVF_EINVAL, args
    assert L.gvf_image_loss_scratch_bytes(1, 8, 8, 0, None) == _lib.GVF_EINVAL


def test_forward_backward_refusals(L):
    """Null pointers and bad geometry are refused on the host; nothing is launched (no GPU here)."""
    from gvfdiffusion_amd import _lib
    buf = ctypes.c_void_p(0)
    fwd = lambda p, g, planes, H, W, t, s, flags=0: L.gvf_image_loss_forward(p, g, planes, H, W, 1.0, 0.2, t, s, 1 << 20, flags, None)  # noqa: E731
    assert fwd(None, None, 1, 8, 8, None, None) == _lib.GVF_EINVAL
    assert fwd(buf, buf, 1, 8, 8, buf, buf) == _lib.GVF_EINVAL           # null device pointers
    bwd = lambda p, g, planes, H, W, gt, gr, s, flags: L.gvf_image_loss_backward(p, g, planes, H, W, 1.0, 0.2, gt, gr, s, 1 << 20, flags, None)  # noqa: E731
    assert bwd(None, None, 1, 8, 8, None, None, None, 0) == _lib.GVF_EINVAL
    assert bwd(None, None, 1, 8, 8, None, None, None, 1) == _lib.GVF_EINVAL


def test_window_taps_are_the_reference_taps(L):
    from gvfdiffusion_amd import _lib
    from gvfdiffusion_amd.ops import image_loss
    assert L.gvf_ssim_window(None) == _lib.GVF_EINVAL
    ref = np.load(GOLDEN)["window1d"]
    assert np.array_equal(image_loss.window_taps().numpy().view(np.uint32), ref.view(np.uint32))


def test_python_refusals_without_gpu():
    from gvfdiffusion_amd import _lib
    from gvfdiffusion_amd.ops import image_loss
    a, b = torch.rand(3, 8, 8), torch.rand(3, 8, 8)
    with pytest.raises(_lib.GvfError):
        image_loss.image_loss(a, b)
    with pytest.raises(_lib.GvfError):
        image_loss.ssim(a, b)
    with pytest.raises(ValueError):
        image_loss.image_loss(a, b.requires_grad_(True))
