"""Generates tests/golden/interp_loss_golden.npz: the reference's own interpolation loss
(train_vae.py:compute_interpolation_loss_delta_interp) recorded in fp32 and, on the same inputs, in float64.

Runs only where the reference checkout is (see make_golden.py); the fixture holds arrays only.  train_vae.py is loaded by path with
throw-away stubs for what it imports at module level and this function never touches (imageio, accelerate, utils.logger,
utils.loss_util, utils.lpips.lpips, model.nn); pytorch3d.ops.knn_points, which it does call, is a brute force with a stable argsort:
squared distances ascending, the lower index first among equals.

Per input set `<s>`: `in.<s>.gs<b>` (P_b, 14), `in.<s>.static_pc` (B, N, 3), `in.<s>.moving_pc` (B, T, N, 3), `in.<s>.output`
(B, T, max P_b, 14).  Per case `<c>`: `<c>.input_set` (the name of its input set), `<c>.params` = [knn_k, adaptive_radius, beta]; results `<c>.loss32|64`, `<c>.est32|64` (B, T, max P_b, 3) and
`<c>.grad32|64` = d loss / d output[..., :3] (the further channels of the gradient are zero and are not stored).
"""
import os

import numpy as np
import torch

from make_golden import OUT, REF, _stub, load_by_path


def knn_points(p1, p2, lengths1=None, K=8):
    d2 = ((p1[:, :, None, :] - p2[:, None, :, :]) ** 2).sum(-1)
    idx = torch.argsort(d2, dim=-1, stable=True)[..., :K]
    return torch.gather(d2, -1, idx), idx, None


def load_train_vae():
    _stub("imageio")
    acc = _stub("accelerate", Accelerator=object)
    acc.utils = _stub("accelerate.utils", DistributedDataParallelKwargs=object)
    p3 = _stub("pytorch3d")
    p3.ops = _stub("pytorch3d.ops", knn_points=knn_points)
    ut = _stub("utils", logger=_stub("utils.logger"))
    ut.loss_util = _stub("utils.loss_util", ssim=None)
    ut.lpips = _stub("utils.lpips")
    ut.lpips.lpips = _stub("utils.lpips.lpips", LPIPS=object)
    mo = _stub("model")
    mo.nn = _stub("model.nn", update_ema=None)
    return load_by_path("ref_train_vae", f"{REF}/train_vae.py")


def inputs(seed, lens, N, T):
    g = torch.Generator().manual_seed(seed)
    B, P = len(lens), max(lens)
    gs = [torch.rand((n, 14), generator=g) - 0.5 for n in lens]
    static_pc = torch.rand((B, N, 3), generator=g) - 0.5
    moving_pc = static_pc[:, None] + 0.05 * torch.randn((B, T, N, 3), generator=g)
    output = 0.05 * torch.randn((B, T, P, 14), generator=g)
    return gs, static_pc, moving_pc, output


def record(fn, gs, static_pc, moving_pc, output, k, adaptive, beta, dtype):
    gs = [x.to(dtype) for x in gs]
    out = output.to(dtype).clone().requires_grad_(True)
    loss, d, est = fn(gs, static_pc.to(dtype), moving_pc.to(dtype), out, len(gs), knn_k=k, adaptive_radius=adaptive, beta=beta)
    assert set(d) == {"deformation_xyz_loss"} and tuple(d["deformation_xyz_loss"].shape) == (1,)
    loss.backward()
    assert float(out.grad[..., 3:].abs().max()) == 0.0
    return loss.detach().numpy(), est.detach().numpy(), out.grad[..., :3].numpy().copy()


def main():
    fn = load_train_vae().compute_interpolation_loss_delta_interp
    base = inputs(21, [150, 97], 300, 5)
    small = inputs(22, [40, 25], 8, 3)
    sets = {"base": base, "small": small}
    cases = {"base": ("base", 8, True, 7.0), "fixed_radius": ("base", 8, False, 7.0), "k4": ("base", 4, True, 7.0),
             "n_eq_k": ("small", 8, True, 7.0)}
    out = {}
    for sname, (gs, static_pc, moving_pc, output) in sets.items():
        for b, x in enumerate(gs):
            out[f"in.{sname}.gs{b}"] = x.numpy()
        out[f"in.{sname}.static_pc"], out[f"in.{sname}.moving_pc"], out[f"in.{sname}.output"] = static_pc.numpy(), moving_pc.numpy(), output.numpy()
    for name, (sname, k, adaptive, beta) in cases.items():
        gs, static_pc, moving_pc, output = sets[sname]
        out[f"{name}.input_set"] = np.asarray(sname)
        out[f"{name}.params"] = np.asarray([k, int(adaptive), beta], dtype=np.float64)
        for tag, dtype in (("32", torch.float32), ("64", torch.float64)):
            loss, est, grad = record(fn, gs, static_pc, moving_pc, output, k, adaptive, beta, dtype)
            out[f"{name}.loss{tag}"], out[f"{name}.est{tag}"], out[f"{name}.grad{tag}"] = loss, est, grad
        print(name, "loss32", float(out[f"{name}.loss32"]), "loss64", float(out[f"{name}.loss64"]))
    path = os.path.join(OUT, "interp_loss_golden.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
