"""Generates tests/golden/ssim_golden.npz by running the REFERENCE's SSIM (utils/loss_util.py:ssim), on CPU, in fp32 and on the
same inputs cast to float64 (the reference then casts its fp32 window to float64: window.type_as(img1)).  Runs only in the build
container, like make_golden.py.  Usage:  python tests/golden/make_ssim_golden.py

Stub: utils/loss_util.py imports `lpips.LPIPS` at module level (VGG weights, not needed by ssim); a throw-away module stands in.

Per case k: img1_k, img2_k (fp32 inputs), ssim32_k / grad32_k (the reference's fp32 mean SSIM and its autograd gradient in
img1), ssim64_k / grad64_k (the same on float64 inputs).  `window1d`: the fp32 taps of gaussian(11, 1.5)."""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

REF = "/root/reference"
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "ssim_golden.npz")

SHAPES = [(2, 3, 37, 53), (1, 3, 5, 7), (4, 3, 24, 24)]


def load_loss_util():
    sys.modules.setdefault("lpips", types.SimpleNamespace(LPIPS=object))
    spec = importlib.util.spec_from_file_location("ref_loss_util", f"{REF}/utils/loss_util.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def flat_pair(rng):
    """64 x 64 pair of piecewise-constant 16 x 16 blocks (sigma = 0 inside, so C2 dominates), with noise on a few blocks only."""
    base = rng.uniform(0.1, 0.9, size=(1, 3, 4, 4)).astype(np.float32)
    a = np.kron(base, np.ones((1, 1, 16, 16), np.float32))
    b = a + rng.uniform(-0.05, 0.05, size=(1, 3, 4, 4)).repeat(16, 2).repeat(16, 3).astype(np.float32)
    b[..., 32:48, 0:16] += rng.normal(0, 0.02, size=(1, 3, 16, 16)).astype(np.float32)
    return a, np.clip(b, 0, 1).astype(np.float32)


def cases():
    rng = np.random.default_rng(20261015)
    out = []
    for s in SHAPES:
        a = rng.uniform(0, 1, size=s).astype(np.float32)
        b = np.clip(a + rng.normal(0, 0.15, size=s), 0, 1).astype(np.float32)
        out.append((a, b))
    out.append(flat_pair(rng))
    return out


def main():
    lu = load_loss_util()
    data = {"window1d": lu.gaussian(11, 1.5).numpy().astype(np.float32)}
    for k, (a, b) in enumerate(cases()):
        data[f"img1_{k}"], data[f"img2_{k}"] = a, b
        for tag, dt in (("32", torch.float32), ("64", torch.float64)):
            x = torch.from_numpy(a).to(dt).requires_grad_(True)
            y = torch.from_numpy(b).to(dt)
            s = lu.ssim(x, y)
            s.backward()
            data[f"ssim{tag}_{k}"] = s.detach().numpy()
            data[f"grad{tag}_{k}"] = x.grad.numpy()
    data["n_cases"] = np.array(len(SHAPES) + 1)
    np.savez_compressed(OUT, **data)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
