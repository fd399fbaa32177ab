"""Data-parallel training step through the differentiable rasteriser operator.

Reference: the render loss of the motion-VAE training loop, train_vae.py:321-352 (decoder output `pred_delta` -> per
camera `renderers["MipGS"].render(static_gs, extrinsics, intrinsics, delta_pc=pred_delta_b)` -> L1 against the ground
truth image -> accelerator.backward), and the optimisation step of train_latent.py:183-225 (backward ->
clip_grad_norm_(params, 1.0) -> opt.step -> zero_grad) under accelerate's DDP, i.e. gradients averaged over the ranks.

Here: one process per GPU, each rank renders ITS samples through gvf_rast_forward / gvf_rast_backward
(gvfdiffusion_amd/rasterizer.py::_RasterizeFn; render_l1_loss) or all views at once through gvf_rast_forward_batched /
gvf_rast_backward_batched (_RasterizeBatchedFn; render_l1_loss_frames, render_loss_frames), and the gradients of the trainable parameters are averaged with bucketed
all-reduces on the default process group -- RCCL over xGMI on an MI355X node (backend "nccl"), gloo in the CPU tests.
The interpolation ("deformation xyz") term of the same step (train_vae.py:304-311, 486-586) is `interpolation_loss`: the KNN search over
the static anchors, the weighted gather of their motion and the masked L1 against the predicted deltas as fused HIP kernels
(ops/knn_interp.py: gvf_knn_interp_weights, gvf_interp_loss_forward / _backward), where the reference needs pytorch3d's knn_points.
Attention trains through its HIP kernels: with grad enabled, model/attention/full_attn.py::scaled_dot_product_attention runs the
inference forward inside an autograd function whose backward is csrc/attn_bwd.hip (ops/attention_grad.py).
The DiT trains here too: `DiT.enable_training()` makes its forward the differentiable one of model/dit_train.py -- LayerNorm + adaLN
modulate, the gated residual and the QK RMSNorm forward and backward as fused HIP kernels (ops/dit_train.py, csrc/dit_train.hip), attention on
the operator above.  The block projections take torch's library GEMMs by default and, with `enable_training(linear="hip")`, this library's
own: forward and input gradient on gvf_gemm, weight and bias gradients in fp32 from csrc/linear_grad.hip (ops/linear_grad.py), each weight
cast once per step; the fused epilogues and row-block launches of the inference path still carry no gradient.  `diffusion_loss` is the loss of train_latent.py:183-207 on model/gaussian_diffusion.py::training_losses, ready for
`train_step` with an ops.optim.FusedAdamW.  The static VAE trains as well: `SparseTransformerVAE.enable_training()` and
`static_vae_loss` (train_vae.py:228,274: `static_vae.training_losses(...)`; model/sparse_voxel_diffusion/sparse_train.py).  So does the
motion VAE: `GSKLTemporalVariationalAutoEncoder.enable_training()` and `motion_vae_loss` (train_vae.py:295-334: KL + interpolation + render
loss on the decoder's `pred_delta`; model/autoencoder_train.py).  `DeltaHead` is the
smallest such module: the decoder's last projection (model/autoencoder.py `to_outputs`) as a plain torch layer over given
per-Gaussian features, producing the (T, P, 14) deltas.
"""
import sys
from typing import Callable, Iterable, List, Optional, Sequence

import torch
import torch.nn as nn
import torch.nn.functional as F


class DeltaHead(nn.Module):
    """(T, P, feat) decoder features -> (T, P, 14) Gaussian deltas [xyz3 | scale3 | rot4 | rgb3 | op1]
    (renderers/gaussian_render.py:155-160 order); zero-initialised so that training starts from the static Gaussians."""

    def __init__(self, feat: int):
        super().__init__()
        self.to_outputs = nn.Linear(feat, 14)
        nn.init.zeros_(self.to_outputs.weight)
        nn.init.zeros_(self.to_outputs.bias)

    def forward(self, feats: torch.Tensor) -> torch.Tensor:
        return self.to_outputs(feats)


def render_l1_loss(render_fn: Callable, gaussian, extrinsics: torch.Tensor, intrinsics: torch.Tensor, deltas: torch.Tensor,
                   targets: torch.Tensor, frame_of_view: Optional[Sequence[int]] = None) -> torch.Tensor:
    """mean_v L1(render(gaussian, cam_v, delta_pc = deltas[frame(v)]), targets[v]) -- train_vae.py:321-330.
    render_fn(gaussian, extrinsics(4,4), intrinsics(3,3), delta_pc(P,14)) -> (3,H,W), differentiable in delta_pc."""
    V = extrinsics.shape[0]
    loss = 0.0
    for v in range(V):
        t = v if frame_of_view is None else int(frame_of_view[v])
        img = render_fn(gaussian, extrinsics[v], intrinsics, deltas[t])
        loss = loss + F.l1_loss(img, targets[v])
    return loss / V


def render_l1_loss_frames(renderer, gaussian, extrinsics: torch.Tensor, intrinsics: torch.Tensor, deltas: torch.Tensor,
                          targets: torch.Tensor, frame_of_view: Optional[Sequence[int]] = None) -> torch.Tensor:
    """render_l1_loss with the V views rendered in ONE renderer.render_frames call (GaussianRenderer: the batched fused-activation
    rasteriser, differentiated by gvf_rast_backward_batched) instead of V single-frame renders: view v uses delta slice
    frame_of_view[v] (default v).  Same loss: mean_v L1(frame_v, targets[v])."""
    V = extrinsics.shape[0]
    index = list(range(V)) if frame_of_view is None else [int(t) for t in frame_of_view]
    imgs = renderer.render_frames(gaussian, extrinsics, intrinsics, delta_pc=deltas, delta_index=index)["rgb"]
    loss = 0.0
    for v in range(V):
        loss = loss + F.l1_loss(imgs[v], targets[v])
    return loss / V


def render_loss_frames(renderer, gaussian, extrinsics: torch.Tensor, intrinsics: torch.Tensor, deltas: torch.Tensor,
                       targets: torch.Tensor, frame_of_view: Optional[Sequence[int]] = None, l1_weight: float = 1.0,
                       ssim_weight: float = 0.2, lpips=None, lpips_weight: float = 0.0) -> torch.Tensor:
    """The reference's render loss (train_vae.py:328-334):
        l1_weight * L1(frames, targets) + ssim_weight * (1 - ssim(frames, targets)) + lpips_weight * lpips(frames * 2 - 1, targets * 2 - 1)
    over the stacked (V, 3, H, W) views, rendered in ONE renderer.render_frames call as in render_l1_loss_frames.  L1 and SSIM are ONE
    fused HIP loss (ops/image_loss.py: gvf_image_loss_forward / _backward); the LPIPS term is added when `lpips` is an ops.lpips.LPIPS
    module (the caller owns it and its weights) and lpips_weight is not zero -- with the defaults the loss is the L1 + SSIM part alone.
    For views of one size, the L1 over the stack equals the mean of the per-view L1s of render_l1_loss_frames."""
    from .ops.image_loss import image_loss
    V = extrinsics.shape[0]
    index = list(range(V)) if frame_of_view is None else [int(t) for t in frame_of_view]
    imgs = renderer.render_frames(gaussian, extrinsics, intrinsics, delta_pc=deltas, delta_index=index)["rgb"]
    loss = image_loss(imgs, targets, l1_weight=l1_weight, ssim_weight=ssim_weight)
    if lpips is not None and lpips_weight != 0.0:
        loss = loss + lpips_weight * lpips(imgs * 2 - 1, targets * 2 - 1)
    return loss


def interpolation_loss(static_gs: Sequence[torch.Tensor], micro_static_pc: torch.Tensor, micro_moving_pc: torch.Tensor, output: torch.Tensor,
                       knn_k: int = 8, adaptive_radius: bool = True, beta: float = 7.0):
    """The reference's interpolation loss (train_vae.py:486-586, compute_interpolation_loss_delta_interp) on the fused HIP operator:
    static_gs is a list of B ragged (P_b, >= 3) Gaussian tensors (xyz first), micro_static_pc (B, N, 3), micro_moving_pc (B, T, N, 3)
    absolute positions, output (B, T, >= max P_b, >= 3) the predicted deltas, of which output[b, :, :P_b, :3] is scored against the
    KNN-interpolated motion of the Gaussians.  Returns (loss, {"deformation_xyz_loss": loss as a detached 1-element tensor},
    estimated_deltas (B, T, max P_b, 3)); the loss is differentiable in output only, and an output whose third dimension equals
    max P_b is read in place (no slice copy)."""
    from .ops.knn_interp import interpolation_l1
    if len(static_gs) == 0 or len(static_gs) != micro_static_pc.shape[0]:
        raise ValueError(f"interpolation_loss: {len(static_gs)} Gaussian sets for {micro_static_pc.shape[0]} samples")
    for g in static_gs:
        if g.dim() != 2 or g.shape[1] < 3:
            raise ValueError(f"interpolation_loss: expected (P_b, >= 3) Gaussians, got {tuple(g.shape)}")
    lengths = [int(g.shape[0]) for g in static_gs]
    P = max(lengths)
    if output.dim() != 4 or output.shape[2] < P:
        raise ValueError(f"interpolation_loss: output {tuple(output.shape)} has fewer than {P} rows per frame")
    with torch.no_grad():
        q = torch.stack([F.pad(g[:, :3].float(), (0, 0, 0, P - g.shape[0])) for g in static_gs])
    pred = output if output.shape[2] == P else output[:, :, :P]
    loss, est = interpolation_l1(pred, q, micro_static_pc, micro_moving_pc, lengths=lengths, k=knn_k, beta=beta,
                                 adaptive_radius=adaptive_radius, return_est=True)
    return loss, {"deformation_xyz_loss": loss.detach().reshape(1)}, est


def diffusion_loss(diffusion, model, latent: torch.Tensor, cond: dict, sampler=None, t: Optional[torch.Tensor] = None,
                   noise: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The diffusion training loss of train_latent.py:183-207: t ~ sampler (model/resample.py; uniform over the diffusion's steps when
    neither `sampler` nor `t` is given), losses = diffusion.training_losses(model, latent, t, model_kwargs=cond, noise), returns
    losses["loss"].mean().  cond holds the model's keyword arguments (cond_images, static_latent, deformation_position_xyz); the
    reference's `mem_ratio` entry (its elastic checkpointing ratio) is not accepted -- set use_checkpoint on the blocks instead.
    The sampler's importance weights are 1 for the uniform sampler and, as in the reference, do not enter the loss."""
    if "mem_ratio" in cond:
        raise ValueError("diffusion_loss: 'mem_ratio' is not a model argument here (no elastic checkpointing); drop it from cond")
    if t is None:
        if sampler is None:
            from .model.resample import UniformSampler
            sampler = UniformSampler(diffusion.num_timesteps)
        t, _ = sampler.sample(latent.shape[0], latent.device)
    losses, _ = diffusion.training_losses(model, latent, t, model_kwargs=cond, noise=noise)
    return losses["loss"].mean()


def static_vae_loss(framework, feats, image: torch.Tensor, extrinsics: torch.Tensor, intrinsics: torch.Tensor, lpips=None,
                    noise: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The static-VAE loss of train_vae.py:228,274: framework.training_losses(...)[0]["loss"] for a SparseVAE whose backbone is on its
    training path (SparseTransformerVAE.enable_training()), ready for `train_step`.  feats: the sparse input features; image (N, 3, H, W)
    targets with their cameras; lpips: the caller's ops.lpips.LPIPS module (required when the framework's lambda_lpips > 0); noise: the
    posterior's draw (None: drawn)."""
    terms, _ = framework.training_losses(feats, image, extrinsics, intrinsics, lpips=lpips, noise=noise)
    return terms["loss"]


def motion_vae_loss(model, renderer, gaussians: Sequence, micro_static_pc: torch.Tensor, micro_delta_pc: torch.Tensor, extrinsics: torch.Tensor,
                    intrinsics: torch.Tensor, targets: torch.Tensor, frame_of_view: Optional[Sequence[Sequence[int]]] = None,
                    kl_weight: float = 1e-5, xyz_loss_weight: float = 0.1, l1_weight: float = 1.0, ssim_weight: float = 0.2, lpips=None,
                    lpips_weight: float = 1.0, knn_k: int = 8, beta: float = 7.0, noise: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The motion-VAE part of the reference's joint step (train_vae.py:295-334, default weights of :40-47) for a
    GSKLTemporalVariationalAutoEncoder on its training route (enable_training()), ready for `train_step`:
        kl.mean() * kl_weight + interpolation_loss * xyz_loss_weight + render loss (L1 + SSIM [+ LPIPS]) of the deformed Gaussians
    gaussians: the B static GaussianModels (their (P_b, 14) tensors are the decoder's queries); micro_static_pc (B, N, 3), micro_delta_pc
    (B, T, N, 3); extrinsics (B, V, 4, 4), intrinsics (3, 3) or (B, 3, 3), targets (B, V, 3, H, W); frame_of_view[b][v]: the frame view v of
    sample b shows (default v).  The LPIPS term needs the caller's ops.lpips.LPIPS module, as in render_loss_frames; the render loss is the
    mean over the samples of each sample's loss over its V views (the reference's loss over the stacked B * V views)."""
    from .utils.points import get_gaussian_tensor
    static_gs = [get_gaussian_tensor(g) for g in gaussians]
    out = model(static_gs, micro_static_pc, micro_delta_pc, noise=noise)
    pred = out["logits"]                                                  # (B, T, max P_b, 14)
    if pred.grad_fn is None:
        raise RuntimeError("motion_vae_loss: the model's output carries no graph (call enable_training() and run with grad enabled)")
    loss = out["kl"].mean() * kl_weight
    moving = micro_static_pc[:, None] + micro_delta_pc
    interp, _, _ = interpolation_loss(static_gs, micro_static_pc, moving, pred, knn_k=knn_k, beta=beta)
    loss = loss + interp * xyz_loss_weight
    B = len(gaussians)
    render = 0.0
    for b in range(B):
        deltas = pred[b, :, :static_gs[b].shape[0]].contiguous()
        render = render + render_loss_frames(renderer, gaussians[b], extrinsics[b], intrinsics if intrinsics.dim() == 2 else intrinsics[b], deltas,
                                             targets[b], None if frame_of_view is None else frame_of_view[b], l1_weight=l1_weight,
                                             ssim_weight=ssim_weight, lpips=lpips, lpips_weight=lpips_weight)
    return loss + render / B


def allreduce_gradients(params: Iterable[torch.nn.Parameter], group=None, bucket_bytes: int = 64 << 20, flat=None) -> int:
    """DDP's gradient averaging, explicit: grads are packed into flat buckets of <= bucket_bytes (few, large collectives:
    a ring all-reduce over xGMI is per-link bound, so small messages waste it), summed over the ranks with
    all_reduce and divided by the world size; parameters without a gradient contribute zeros, so every rank issues the
    same collectives.  Returns the number of collectives.  No-op when torch.distributed is not initialised.
    flat: an ops.optim.FlatGrads that owns(params) -- the gradients already ARE one flat buffer, which is all-reduced in place in
    slices of <= bucket_bytes (no cat, no copy back) and divided by the world size; returns the number of slices."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()):
        return 0
    world = dist.get_world_size(group)
    plist: List[torch.nn.Parameter] = [p for p in params if p.requires_grad]
    if flat is not None and flat.owns(plist):
        n_coll = 0
        for buf in flat.buffers.values():
            per = max(1, bucket_bytes // buf.element_size())
            for a in range(0, buf.numel(), per):
                dist.all_reduce(buf[a:a + per], op=dist.ReduceOp.SUM, group=group)
                n_coll += 1
            buf.div_(world)
        return n_coll
    n_coll, i = 0, 0
    while i < len(plist):
        bucket, nbytes = [], 0
        dtype, dev = plist[i].dtype, plist[i].device
        while i < len(plist) and plist[i].dtype == dtype and plist[i].device == dev and (not bucket or nbytes + plist[i].numel() * plist[i].element_size() <= bucket_bytes):
            bucket.append(plist[i]); nbytes += plist[i].numel() * plist[i].element_size(); i += 1
        flat = torch.cat([(p.grad if p.grad is not None else torch.zeros_like(p)).reshape(-1) for p in bucket])
        dist.all_reduce(flat, op=dist.ReduceOp.SUM, group=group)
        flat.div_(world)
        off = 0
        for p in bucket:
            g = flat[off:off + p.numel()].view_as(p)
            if p.grad is None:
                p.grad = g.clone()
            else:
                p.grad.copy_(g)
            off += p.numel()
        n_coll += 1
    return n_coll


def train_step(params: Sequence[torch.nn.Parameter], optimizer: torch.optim.Optimizer, loss_fn: Callable[[], torch.Tensor],
               max_grad_norm: float = 1.0, group=None) -> dict:
    """zero_grad -> loss = loss_fn() on this rank's samples -> backward -> gradient all-reduce (mean over ranks) ->
    clip_grad_norm_(max_grad_norm) -> optimizer.step   (train_latent.py:183-215).
    With an ops.optim.FusedAdamW the norm, the clip, the AdamW update and the EMAs are the optimizer's one fused device-side step
    (optimizer.max_grad_norm is set from the argument), the all-reduce runs in place on its flat gradient buffer, and the returned
    dict has a further key "found_inf" (1: a non-finite gradient norm, the step was skipped on the device)."""
    fused = sys.modules.get(__package__ + ".ops.optim")    # never imported: the optimizer cannot be one of its class, and the old path imports nothing
    if fused is not None and isinstance(optimizer, fused.FusedAdamW):
        optimizer.zero_grad()
        loss = loss_fn()
        loss.backward()
        n = allreduce_gradients(params, group=group, flat=optimizer.flat_grads)
        optimizer.max_grad_norm = max_grad_norm
        optimizer.step()
        return {"loss": float(loss.detach()), "grad_norm": float(optimizer.grad_norm), "collectives": n,
                "found_inf": int(optimizer.found_inf)}
    optimizer.zero_grad(set_to_none=True)
    loss = loss_fn()
    loss.backward()
    n = allreduce_gradients(params, group=group)
    gnorm = torch.nn.utils.clip_grad_norm_(list(params), max_grad_norm)
    optimizer.step()
    return {"loss": float(loss.detach()), "grad_norm": float(gnorm), "collectives": n}
