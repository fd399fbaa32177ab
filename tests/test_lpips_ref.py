"""The fp64 LPIPS helper (tests/lpips_ref.py) against the reference's own code (tests/golden/lpips_golden.npz, written by
tests/golden/make_lpips_golden.py) and against itself: finite differences, lpips(x, x) = 0, symmetry.  No GPU."""
import os

import numpy as np
import pytest
import torch

import lpips_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lpips_golden.npz")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def weights(golden):
    return R.seeded_weights(int(golden["seed"]))


def test_seeded_weights_are_the_reference_state_dict(weights):
    from gvfdiffusion_amd.ops.lpips import LPIPS
    assert set(weights) == set(LPIPS().state_dict())
    w = weights["net.layers.28.weight"]
    assert w.shape == (512, 512, 3, 3) and abs(float(w.mean())) < 1e-3 and float(w.abs().max()) <= (6 / (9 * 512)) ** 0.5
    assert all(float(weights[f"lin.{t}.1.weight"].min()) >= 0 for t in range(5))
    # a counter-based hash, not a library stream: the first values are these on every machine
    assert R.hash_uniform(7, 0, 2).tolist() == [0.22309773791404108, 0.2956474228481226]


def test_helper_matches_the_reference_code(golden, weights):
    for k in range(int(golden["n_cases"])):
        x, y = torch.from_numpy(golden[f"x_{k}"]), torch.from_numpy(golden[f"y_{k}"])
        loss, grad = R.loss_and_grad(x, y, weights)
        gl, gg = float(golden[f"loss_{k}"]), torch.from_numpy(golden[f"grad_{k}"])
        assert abs(float(loss) - gl) <= 1e-9 * abs(gl), (k, float(loss), gl)
        rel = float((grad - gg).norm() / gg.norm())
        print(f"case {k}: loss {float(loss):.12g} golden {gl:.12g}, gradient rel L2 {rel:.2e}")
        assert rel <= 1e-9, k


def test_directional_finite_differences(golden, weights):
    """Eight random directions, central differences with h = 1e-5 and 1e-6 on 37 x 50 against the analytic fp64 gradient; bar 1e-4 (measured
    worst: 5.1e-6)."""
    x, y = torch.from_numpy(golden["x_0"]).double(), torch.from_numpy(golden["y_0"]).double()
    _, grad = R.loss_and_grad(x, y, weights)
    worst = 0.0
    with torch.no_grad():
        for d in range(8):
            v = torch.from_numpy(R.hash_uniform(31, d, x.numel()) * 2 - 1).reshape(x.shape)
            v = v / v.norm()
            want = float((grad * v).sum())
            h = 1e-5 if d % 2 == 0 else 1e-6
            fd = float(R.lpips(x + h * v, y, weights) - R.lpips(x - h * v, y, weights)) / (2 * h)
            worst = max(worst, abs(fd - want) / abs(want))
    print(f"finite differences: worst relative deviation {worst:.2e}")
    assert worst <= 1e-4


def test_equal_images_give_zero_and_zero_gradient(golden, weights):
    x = torch.from_numpy(golden["x_1"])
    loss, grad = R.loss_and_grad(x, x.clone(), weights)
    assert float(loss) == 0.0 and float(grad.abs().max()) == 0.0


def test_symmetry(golden, weights):
    x, y = torch.from_numpy(golden["x_1"]), torch.from_numpy(golden["y_1"])
    with torch.no_grad():
        a, b = float(R.lpips(x, y, weights)), float(R.lpips(y, x, weights))
    assert a > 0 and abs(a - b) <= 1e-14 * a
