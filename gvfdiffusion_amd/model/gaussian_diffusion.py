"""The part of the reference's guided-diffusion heritage this package needs: the beta schedule that feeds NoiseScheduleVP
(inference_dpm_latent.py:75,156 -> utils/script_util.py:7-61 -> model/gaussian_diffusion.py:35-89) and the diffusion training loss of
train_latent.py:183-207 (model/gaussian_diffusion.py:233-277, 418-421, 781-862): q_sample, the eps / xstart / v targets, the MSE term and
its min-SNR weight.  Learned-sigma / KL losses and timestep respacing stay out of scope (no released config uses them): they raise."""
import math

import numpy as np
import torch


def betas_for_alpha_bar(num_diffusion_timesteps, alpha_bar, max_beta=0.999):
    """beta_i = min(1 - abar((i+1)/T) / abar(i/T), max_beta), float64."""
    T = num_diffusion_timesteps
    return np.array([min(1 - alpha_bar((i + 1) / T) / alpha_bar(i / T), max_beta) for i in range(T)])


def get_named_beta_schedule(schedule_name, num_diffusion_timesteps, beta_start=0.0001, beta_end=0.02):
    if schedule_name == "linear":
        scale = 1000 / num_diffusion_timesteps
        return np.linspace(scale * beta_start, scale * beta_end, num_diffusion_timesteps, dtype=np.float64)
    if schedule_name == "cosine":
        return betas_for_alpha_bar(num_diffusion_timesteps, lambda t: math.cos((t + 0.008) / 1.008 * math.pi / 2) ** 2)
    raise NotImplementedError(f"unknown beta schedule: {schedule_name}")


def _extract_into_tensor(arr, timesteps, broadcast_shape):
    """arr[timesteps] of a float64 numpy table as fp32, broadcast to `broadcast_shape` (model/gaussian_diffusion.py:936-948)."""
    res = torch.from_numpy(arr).to(device=timesteps.device)[timesteps].float()
    while len(res.shape) < len(broadcast_shape):
        res = res[..., None]
    return res.expand(broadcast_shape)


def mean_flat(tensor):
    return tensor.mean(dim=list(range(1, len(tensor.shape))))


class GaussianDiffusion:
    """`.betas` (what inference reads, inference_dpm_latent.py:156) and the training loss (training_losses)."""

    def __init__(self, betas, predict_type="eps", rescale_timesteps=False, min_snr=False, learn_sigma=False, use_kl=False):
        self.betas = np.asarray(betas, dtype=np.float64)
        self.num_timesteps = int(self.betas.shape[0])
        self.predict_type = predict_type
        self.rescale_timesteps = rescale_timesteps
        self.min_snr = min_snr
        self.learn_sigma = learn_sigma
        self.use_kl = use_kl
        # float64 tables, extracted to fp32 per use (model/gaussian_diffusion.py:167-175)
        self.alphas_cumprod = np.cumprod(1.0 - self.betas, axis=0)
        self.sqrt_alphas_cumprod = np.sqrt(self.alphas_cumprod)
        self.sqrt_one_minus_alphas_cumprod = np.sqrt(1.0 - self.alphas_cumprod)

    def q_sample(self, x_start, t, noise=None):
        """x_t ~ q(x_t | x_0) = sqrt(abar_t) x_0 + sqrt(1 - abar_t) noise; t: integer steps [B]."""
        if noise is None:
            noise = torch.randn_like(x_start)
        assert noise.shape == x_start.shape
        return (_extract_into_tensor(self.sqrt_alphas_cumprod, t, x_start.shape) * x_start
                + _extract_into_tensor(self.sqrt_one_minus_alphas_cumprod, t, x_start.shape) * noise)

    def get_v(self, x, noise, t):
        return (_extract_into_tensor(self.sqrt_alphas_cumprod, t, x.shape) * noise
                - _extract_into_tensor(self.sqrt_one_minus_alphas_cumprod, t, x.shape) * x)

    def _scale_timesteps(self, t):
        if self.rescale_timesteps:
            return t.float() * (1000.0 / self.num_timesteps)
        return t

    def training_losses(self, model, x_start, t, model_kwargs=None, noise=None):
        """The reference's contract: (terms, {"x_t", "model_output"}) with terms["mse"] = mean over all but the batch dimension of
        (target - model(x_t, t, **model_kwargs))^2 and terms["loss"] = terms["mse"] * weight, weight = min(SNR_t, 5) (1 where SNR_t is 0)
        with min_snr, else 1.  t: integer steps [B]."""
        if self.learn_sigma or self.use_kl:
            raise NotImplementedError("learned-sigma / KL diffusion losses are not built (configs/diffusion.yml: learn_sigma false, MSE loss)")
        if model_kwargs is None:
            model_kwargs = {}
        if noise is None:
            noise = torch.randn_like(x_start)
        x_t = self.q_sample(x_start, t, noise=noise)
        if self.min_snr:
            alpha = _extract_into_tensor(self.sqrt_alphas_cumprod, t, t.shape)
            sigma = _extract_into_tensor(self.sqrt_one_minus_alphas_cumprod, t, t.shape)
            snr = (alpha / sigma) ** 2
            mse_loss_weight = torch.stack([snr, 5.0 * torch.ones_like(t)], dim=1).min(dim=1)[0]
            mse_loss_weight[snr == 0] = 1.0
        else:
            mse_loss_weight = torch.ones_like(t)
        model_output = model(x_t, self._scale_timesteps(t), **model_kwargs)
        if self.predict_type == "eps":
            target = noise
        elif self.predict_type == "xstart":
            target = x_start
        else:
            target = self.get_v(x_start, noise, t)
        assert model_output.shape == target.shape == x_start.shape
        terms = {"mse": mean_flat((target - model_output) ** 2)}
        terms["loss"] = terms["mse"] * mse_loss_weight
        return terms, {"x_t": x_t, "model_output": model_output}


def create_gaussian_diffusion(*, steps=1000, learn_sigma=False, sigma_small=False, noise_schedule="linear", use_kl=False,
                              predict_type="eps", predict_xstart=False, rescale_timesteps=False,
                              rescale_learned_sigmas=False, timestep_respacing="", beta_start=0.0001, beta_end=0.02,
                              min_snr=False):
    """Same keyword surface as utils/script_util.py:7-23 (configs/diffusion.yml `diffusion:` splats into it)."""
    if predict_type not in ("eps", "xstart", "v"):
        raise ValueError(f"Unknown predict_type for diffusion model: {predict_type}")
    betas = get_named_beta_schedule(noise_schedule, steps, beta_start, beta_end)
    # The reference wraps the schedule in SpacedDiffusion (model/respace.py:120-134), which re-derives
    # the betas of the retained timesteps from the cumulative products: beta_i = 1 - abar_i / abar_{i-1}.
    # With every step retained that is the same schedule up to float64 rounding; reproduce it bit for bit.
    if timestep_respacing not in ("", None) and list(timestep_respacing) != [steps]:
        raise NotImplementedError("timestep respacing is not built (no released config spaces the training or sampling steps)")
    alphas_cumprod = np.cumprod(1.0 - betas, axis=0)
    new_betas, last = [], 1.0
    for acp in alphas_cumprod:
        new_betas.append(1 - acp / last)
        last = acp
    return GaussianDiffusion(np.array(new_betas), predict_type=predict_type, rescale_timesteps=rescale_timesteps, min_snr=min_snr,
                             learn_sigma=learn_sigma, use_kl=use_kl)
