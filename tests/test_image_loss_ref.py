"""The float64 SSIM oracle (tests/ssim_ref.py) against the reference's own SSIM (tests/golden/ssim_golden.npz, written by
make_ssim_golden.py from utils/loss_util.py) and against central finite differences.  CPU only."""
import os

import numpy as np
import pytest
import torch

import ssim_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ssim_golden.npz")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def _rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def test_window_is_the_reference_window(golden):
    assert torch.equal(ssim_ref.taps32(), torch.from_numpy(golden["window1d"]))
    assert abs(float(ssim_ref.taps32().double().sum()) - 1.0) < 1e-6


@pytest.mark.parametrize("k", range(4))
def test_oracle_matches_reference_fp64(golden, k):
    a = torch.from_numpy(golden[f"img1_{k}"]).double().requires_grad_(True)
    b = torch.from_numpy(golden[f"img2_{k}"]).double()
    s = ssim_ref.ssim64(a, b)
    s.backward()
    assert abs(float(s) - float(golden[f"ssim64_{k}"])) <= 1e-12, (float(s), float(golden[f"ssim64_{k}"]))
    e = _rel_l2(a.grad.numpy(), golden[f"grad64_{k}"])
    assert e <= 1e-10, e
    # the fp32 torch composition is the same formula (sanity of the yardstick the device tests use)
    s32 = ssim_ref.ssim_torch32(a.detach().float(), b.float())
    assert abs(float(s32) - float(golden[f"ssim64_{k}"])) < 1e-4


def test_oracle_gradient_matches_finite_differences():
    g = torch.Generator().manual_seed(3)
    a = torch.rand(1, 2, 9, 13, generator=g, dtype=torch.float64)
    b = (a + 0.2 * torch.randn(a.shape, generator=g, dtype=torch.float64)).clamp(0, 1)
    x = a.clone().requires_grad_(True)
    ssim_ref.loss64(x, b, 1.0, 0.2).backward()
    h = 1e-6
    for idx in [(0, 0, 0, 0), (0, 1, 4, 6), (0, 0, 8, 12), (0, 1, 2, 11), (0, 0, 5, 0)]:
        xp, xm = a.clone(), a.clone()
        xp[idx] += h
        xm[idx] -= h
        fd = (float(ssim_ref.loss64(xp, b)) - float(ssim_ref.loss64(xm, b))) / (2 * h)
        assert abs(fd - float(x.grad[idx])) <= 1e-6 * max(1.0, abs(fd)), (idx, fd, float(x.grad[idx]))


def test_oracle_identical_images():
    a = torch.rand(2, 3, 20, 17, dtype=torch.float64)
    x = a.clone().requires_grad_(True)
    s = ssim_ref.ssim64(x, a)
    s.backward()
    assert abs(float(s) - 1.0) < 1e-14
    assert float(x.grad.abs().max()) < 1e-12
