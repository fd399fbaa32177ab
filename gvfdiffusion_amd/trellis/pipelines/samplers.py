"""Euler samplers of the rectified-flow models (trellis/pipelines/samplers/flow_euler.py:11-199 with its two guidance mixins),
`sample_sparse_structure` (trellis/pipelines/trellis_image_to_3d.py:165-196): noise on the dense latent grid -> the coordinates of the
occupied cells, `sample_slat` (:238-253): noise on those coordinates -> the de-normalised structured latent, and `tokens_to_gaussians`,
which chains the two with the structured-latent Gaussian decoder.  Same `sample(...)` arguments and returned fields (`samples`, `pred_x_t`, `pred_x_0`); the state is a SparseTensor or a
dense tensor -- only `+`, `-` and scalar `*` are used on it -- and the result is an attrdict in place of easydict.

The flow:  x_t = (1 - t) x_0 + (sigma_min + (1 - sigma_min) t) eps,  the model predicts v = d x_t / d t = (1 - sigma_min) eps - x_0,
one step is  x_{t'} = x_t - (t - t') v,  and t runs over  rescale_t s / (1 + (rescale_t - 1) s)  for s = 1 ... 0 in `steps` equal parts.
The model is called with 1000 t, once per sample of the batch.  Guidance: v = (1 + w) v(cond) - w v(neg_cond); the interval sampler
applies it only while cfg_interval[0] <= t <= cfg_interval[1] and calls the model once outside."""
from typing import *

import numpy as np
import torch

from ... import sparse as sp
from ...attrdict import AttrDict

__all__ = ["FlowEulerSampler", "FlowEulerCfgSampler", "FlowEulerGuidanceIntervalSampler", "sample_slat", "sample_sparse_structure",
           "tokens_to_gaussians"]


class FlowEulerSampler:
    def __init__(self, sigma_min: float):
        self.sigma_min = sigma_min

    # ---- the parametrisations of one prediction --------------------------------------------------------------------------------------
    def _noise_scale(self, t):
        return self.sigma_min + (1 - self.sigma_min) * t

    def _eps_to_xstart(self, x_t, t, eps):
        return (x_t - self._noise_scale(t) * eps) / (1 - t)

    def _xstart_to_eps(self, x_t, t, x_0):
        return (x_t - (1 - t) * x_0) / self._noise_scale(t)

    def _v_to_xstart_eps(self, x_t, t, v):
        return (1 - self.sigma_min) * x_t - self._noise_scale(t) * v, (1 - t) * v + x_t

    # ---- the model call ------------------------------------------------------------------------------------------------------------------
    def _call(self, model, x_t, t, cond, **kwargs):
        ts = torch.full((x_t.shape[0],), 1000.0 * float(t), dtype=torch.float32, device=x_t.device)
        return model(x_t, ts, cond, **kwargs)

    def _velocity(self, model, x_t, t, cond=None, **kwargs):
        """The velocity the step uses; the guided samplers override this."""
        return self._call(model, x_t, t, cond, **kwargs)

    @torch.no_grad()
    def sample_once(self, model, x_t, t: float, t_prev: float, cond: Optional[Any] = None, **kwargs):
        v = self._velocity(model, x_t, t, cond, **kwargs)
        x_0, _ = self._v_to_xstart_eps(x_t, t, v)
        return AttrDict(pred_x_prev=x_t - (t - t_prev) * v, pred_x_0=x_0)

    @staticmethod
    def timesteps(steps: int, rescale_t: float = 1.0) -> np.ndarray:
        s = np.linspace(1, 0, steps + 1)
        return rescale_t * s / (1 + (rescale_t - 1) * s)

    @torch.no_grad()
    def sample(self, model, noise, cond: Optional[Any] = None, steps: int = 50, rescale_t: float = 1.0, verbose: bool = True, **kwargs):
        ts = self.timesteps(steps, rescale_t)
        ret = AttrDict(samples=None, pred_x_t=[], pred_x_0=[])
        x = noise
        for t, t_prev in zip(ts[:-1], ts[1:]):
            out = self.sample_once(model, x, float(t), float(t_prev), cond, **kwargs)
            x = out.pred_x_prev
            ret.pred_x_t.append(x)
            ret.pred_x_0.append(out.pred_x_0)
        ret.samples = x
        return ret


class FlowEulerCfgSampler(FlowEulerSampler):
    """Euler sampling with classifier-free guidance at every step."""

    def _velocity(self, model, x_t, t, cond, neg_cond, cfg_strength, **kwargs):
        pos = self._call(model, x_t, t, cond, **kwargs)
        neg = self._call(model, x_t, t, neg_cond, **kwargs)
        return (1 + cfg_strength) * pos - cfg_strength * neg

    @torch.no_grad()
    def sample(self, model, noise, cond, neg_cond, steps: int = 50, rescale_t: float = 1.0, cfg_strength: float = 3.0, verbose: bool = True,
               **kwargs):
        return super().sample(model, noise, cond, steps, rescale_t, verbose, neg_cond=neg_cond, cfg_strength=cfg_strength, **kwargs)


class FlowEulerGuidanceIntervalSampler(FlowEulerSampler):
    """Euler sampling with classifier-free guidance inside a time interval, the plain conditional velocity outside it."""

    def _velocity(self, model, x_t, t, cond, neg_cond, cfg_strength, cfg_interval, **kwargs):
        pos = self._call(model, x_t, t, cond, **kwargs)
        if not (cfg_interval[0] <= t <= cfg_interval[1]):
            return pos
        neg = self._call(model, x_t, t, neg_cond, **kwargs)
        return (1 + cfg_strength) * pos - cfg_strength * neg

    @torch.no_grad()
    def sample(self, model, noise, cond, neg_cond, steps: int = 50, rescale_t: float = 1.0, cfg_strength: float = 3.0,
               cfg_interval: Tuple[float, float] = (0.0, 1.0), verbose: bool = True, **kwargs):
        return super().sample(model, noise, cond, steps, rescale_t, verbose, neg_cond=neg_cond, cfg_strength=cfg_strength,
                              cfg_interval=cfg_interval, **kwargs)


@torch.no_grad()
def sample_slat(flow_model, cond: torch.Tensor, neg_cond: torch.Tensor, coords: torch.Tensor, sampler_params: Optional[dict] = None,
                normalization: Optional[dict] = None, noise: Optional[torch.Tensor] = None, sampler=None, **model_kwargs) -> sp.SparseTensor:
    """coords int32 (T, 4) of the sparse structure + the image-condition tokens -> the structured latent (T, out_channels), de-normalised
    with normalization["std"] / ["mean"] -- the input of SLatGaussianDecoder.  sampler_params: steps, cfg_strength, cfg_interval,
    rescale_t of FlowEulerGuidanceIntervalSampler (sigma_min 1e-5, the released pipeline's); noise: (T, in_channels), default drawn here."""
    device = coords.device
    if noise is None:
        noise = torch.randn((coords.shape[0], flow_model.in_channels)).to(device)
    x = sp.SparseTensor(feats=noise.to(device), coords=coords)
    sampler = FlowEulerGuidanceIntervalSampler(sigma_min=1e-5) if sampler is None else sampler
    slat = sampler.sample(flow_model, x, cond=cond, neg_cond=neg_cond, verbose=False, **(sampler_params or {}), **model_kwargs).samples
    if normalization is not None:
        std = torch.tensor(normalization["std"], dtype=slat.feats.dtype)[None].to(device)
        mean = torch.tensor(normalization["mean"], dtype=slat.feats.dtype)[None].to(device)
        slat = slat * std + mean
    return slat


@torch.no_grad()
def sample_sparse_structure(flow_model, decoder, cond: torch.Tensor, neg_cond: torch.Tensor, num_samples: int = 1,
                            sampler_params: Optional[dict] = None, noise: Optional[torch.Tensor] = None, sampler=None,
                            **model_kwargs) -> torch.Tensor:
    """The image-condition tokens -> int32 coords (n, 4) = (b, x, y, z) of the sparse structure, on the device and in row order: a guided
    Euler run of SparseStructureFlowModel over the dense latent, SparseStructureDecoder on its rows, and the cells whose logit is > 0 --
    torch.argwhere(decoder(z_s) > 0)[:, [0, 2, 3, 4]].  sampler_params: steps, cfg_strength, cfg_interval, rescale_t of
    FlowEulerGuidanceIntervalSampler (sigma_min 1e-5, the released pipeline's); noise: (num_samples, in_channels, R, R, R), default drawn
    here as the reference draws it.  model_kwargs (`ops=`) go to both models."""
    from ..models.sparse_structure_vae import to_rows
    from ..models.structured_latent_flow import HipOps
    device = cond.device
    R = flow_model.resolution
    if noise is None:
        noise = torch.randn(num_samples, flow_model.in_channels, R, R, R).to(device)
    sampler = FlowEulerGuidanceIntervalSampler(sigma_min=1e-5) if sampler is None else sampler
    z_s = sampler.sample(flow_model, noise.to(device), cond=cond, neg_cond=neg_cond, verbose=False, **(sampler_params or {}), **model_kwargs).samples
    ops = model_kwargs.get("ops")
    B = z_s.shape[0]
    logits, grid = decoder.forward_rows(to_rows(z_s).float(), (B, R, R, R), ops)
    if logits.shape[1] != 1:
        raise ValueError(f"the sparse structure is read from ONE occupancy logit per cell, the decoder has {logits.shape[1]} output channels")
    occupancy = HipOps.occupancy if ops is None else ops.occupancy
    return occupancy(logits.reshape(B, -1).contiguous(), grid)


@torch.no_grad()
def tokens_to_gaussians(models: dict, cond: torch.Tensor, neg_cond: torch.Tensor, num_samples: int = 1,
                        sparse_structure_sampler_params: Optional[dict] = None, slat_sampler_params: Optional[dict] = None,
                        slat_normalization: Optional[dict] = None, noise: Optional[torch.Tensor] = None, **model_kwargs):
    """The TRELLIS half from the DINOv2 tokens on: sample_sparse_structure -> sample_slat -> SLatGaussianDecoder.  models: the reference
    pipeline's names -- "sparse_structure_flow_model", "sparse_structure_decoder", "slat_flow_model", "slat_decoder_gs".  -> (the decoder's
    Gaussians, the structured latent, the coords).  noise: the sparse-structure stage's, default drawn there."""
    coords = sample_sparse_structure(models["sparse_structure_flow_model"], models["sparse_structure_decoder"], cond, neg_cond, num_samples,
                                     sparse_structure_sampler_params, noise=noise, **model_kwargs)
    if coords.shape[0] == 0:
        raise ValueError("the sparse structure is empty: no cell of the decoder's grid has a positive occupancy logit")
    slat = sample_slat(models["slat_flow_model"], cond, neg_cond, coords, slat_sampler_params, slat_normalization, **model_kwargs)
    return models["slat_decoder_gs"](slat), slat, coords
